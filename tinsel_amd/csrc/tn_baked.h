// tn_baked.h -- the flat scan and the light tables of a BAKED build: one scene's wave-uniform level as compile-time constants.
//
// A baked translation unit (TN_BAKED_HEADER, tn_scene.h) includes a generated header that states, in namespace tn::baked and as 32-bit
// words (floats by their bit patterns, never as decimal literals):
//   kNumPrims, kNumPlanes, kPlanePairEnd, kPlaneSlots, kScanMask      DevScene's counts and the scan's primitive mask
//   kPlaneEq[kPlaneSlots*4], kPlaneIdx[kPlaneSlots]                   the plane table (DevScene::planeEq / planeIdx)
//   kBoxes[kNumPrims*8]                                               the leaf boxes (PrimBox)
//   kPrims[kNumPrims*16]                                              the primitive records (Prim64)
//   kNumLights, kTotalLightSamples, kLights[kNumLights*4]             LightRec: primitive, samples, 1/samples, 0
//   kLightMat[kNumLights*4]                                           the light's own Mat128 words: rcpArea, cbsdf, clight, rcpLightSamples
// trace_flat_baked below is trace_flat (tn_isect.h) over those constants: the same tests, by the same leaf functions, on the same operands, in
// the same order -- unrolled over compile-time slots and primitives, so that a slot's kind, a primitive's type and flags and the table's shape
// are decided by the compiler and nothing of the scene level is fetched or held in scalar registers.  What depends on the ray stays at run
// time: a pair with both planes ahead, non-finite rays, the tie re-trace through the BVH walk (trace), pose_rotate's zero-component branch.
// Only the closed FIT instance of k_bounce takes this path (SceneT::kBaked); the host launches it only for the scene whose key it was
// compiled from (tn_host_bake.h).  tests/test_gpu_bake.py (cornell and its edits) and tests/test_gpu_closed_corpus.py (every form of the
// light tables, no plane table, sixteen slots, a remainder slot, primitive 63, rotated and scaled poses) hold it to the library's instance
// bit for bit.
#pragma once

#if TN_BAKED_SCENE

namespace tn {
namespace baked {

TN_D constexpr float word_f(uint32_t bits) { return __builtin_bit_cast(float, bits); }

template <int K> struct Slot { static constexpr int v = K; };
template <int B, int E, class F>
TN_D void static_for(F&& fn)
{
    if constexpr (B < E)
    {
        fn(Slot<B>());
        static_for<B + 1, E>(fn);
    }
}

template <int S> TN_D ConstF4V plane_eq()
{
    static_assert(S >= 0 && S < kPlaneSlots, "a slot of the plane table");
    return ConstF4V{ word_f(kPlaneEq[S*4]), word_f(kPlaneEq[S*4 + 1]), word_f(kPlaneEq[S*4 + 2]), word_f(kPlaneEq[S*4 + 3]) };
}

template <int I> TN_D Prim64 prim()
{
    static_assert(I >= 0 && I < kNumPrims, "a primitive of the scene");
    constexpr int w = I*16;
    Prim64 p;
    p.px = word_f(kPrims[w]); p.py = word_f(kPrims[w + 1]); p.pz = word_f(kPrims[w + 2]); p.s = word_f(kPrims[w + 3]);
    p.rx = word_f(kPrims[w + 4]); p.ry = word_f(kPrims[w + 5]); p.rz = word_f(kPrims[w + 6]); p.rw = word_f(kPrims[w + 7]);
    p.g0 = word_f(kPrims[w + 8]); p.g1 = word_f(kPrims[w + 9]); p.g2 = word_f(kPrims[w + 10]); p.g3 = word_f(kPrims[w + 11]);
    p.type = kPrims[w + 12]; p.flags = kPrims[w + 13]; p.mesh = kPrims[w + 14]; p.moving = kPrims[w + 15];
    return p;
}

// The record of light primitive `index` (primitive_sample's).  Every active lane of a light loop samples the same light; with one light the
// record is that light's constants, with a few the lanes select among them, and past that the record is loaded as the library does.
constexpr int kLightSelectMax = 4;
template <class SC> TN_D Prim64 light_prim(const SC& sc, int index)
{
    if constexpr (kNumLights >= 1 && kNumLights <= kLightSelectMax)
    {
        Prim64 p = prim<(int)kLights[0]>();
        static_for<1, kNumLights>([&](auto l) {
            constexpr int k = (int)kLights[decltype(l)::v*4];
            if (index == k)
                p = prim<k>();
        });
        return p;
    }
    else
        return load_prim(sc.prims, index);
}

// a light's own Mat128 words, by the same rule
struct LightMat
{
    int light;
    const Mat128* mats;
    template <int W> TN_D float word(float loaded) const
    {
        if constexpr (kNumLights >= 1 && kNumLights <= kLightSelectMax)
        {
            float x = word_f(kLightMat[W]);
            static_for<1, kNumLights>([&](auto l) {
                if (light == (int)kLights[decltype(l)::v*4])
                    x = word_f(kLightMat[decltype(l)::v*4 + W]);
            });
            return x;
        }
        else
            return loaded;
    }
    TN_D float rcpArea() const { return word<0>(mats[light].rcpArea); }
    TN_D float cbsdf() const { return word<1>(mats[light].cbsdf); }
    TN_D float clight() const { return word<2>(mats[light].clight); }
};

// LightCursor::next and nee_sum's loop bounds (tn_integrator.h) from the light table
struct LightCursor
{
    int li = 0, sInLight = 0;
    TN_D int next()
    {
        while (sInLight >= (int)kLights[li*4 + 1]) { ++li; sInLight = 0; }
        ++sInLight;
        return (int)kLights[li*4];
    }
};

// the single planes of the table from slot FROM on: four at a time, then one after the other (trace_flat's kCompactSingles form)
template <int FROM, class Accept>
TN_D void single_planes(V3 o, V3 d, Accept& accept)
{
    constexpr int blocks = kNumPlanes > FROM ? (kNumPlanes - FROM)/4 : 0;
    static_for<0, blocks>([&](auto b) {
        constexpr int pk = FROM + 4*decltype(b)::v;
        const ConstF4V e0 = plane_eq<pk>(), e1 = plane_eq<pk + 1>(), e2 = plane_eq<pk + 2>(), e3 = plane_eq<pk + 3>();
        float t0, t1, t2, t3;
        const bool h0 = ray_plane(o, d, e0.x, e0.y, e0.z, e0.w, t0);
        const bool h1 = ray_plane(o, d, e1.x, e1.y, e1.z, e1.w, t1);
        const bool h2 = ray_plane(o, d, e2.x, e2.y, e2.z, e2.w, t2);
        const bool h3 = ray_plane(o, d, e3.x, e3.y, e3.z, e3.w, t3);
        if (h0) accept((int)kPlaneIdx[pk], t0, V3(e0.x, e0.y, e0.z));
        if (h1) accept((int)kPlaneIdx[pk + 1], t1, V3(e1.x, e1.y, e1.z));
        if (h2) accept((int)kPlaneIdx[pk + 2], t2, V3(e2.x, e2.y, e2.z));
        if (h3) accept((int)kPlaneIdx[pk + 3], t3, V3(e3.x, e3.y, e3.z));
    });
    static_for<FROM + 4*blocks, kNumPlanes>([&](auto s) {
        constexpr int pk = decltype(s)::v;
        const ConstF4V e0 = plane_eq<pk>();
        float t0;
        if (ray_plane(o, d, e0.x, e0.y, e0.z, e0.w, t0))
            accept((int)kPlaneIdx[pk], t0, V3(e0.x, e0.y, e0.z));
    });
}

} // namespace baked

// trace_flat for the closed FIT instance (no deferred walks, no any-hit stop, kCompactSingles) over the baked scene level
template <class SC, class Stack, bool COUNT>
TN_D int trace_flat_baked(const SC& sc, Stack& st, V3 o, V3 d, V3 rcp, float time, float& outT, V3& outN, bool& tie, TraceCounters& ctr)
{
    static_assert(SC::kBaked && SC::kDefer == 0 && SC::kFeatures != kFeatAll, "the closed FIT instance");
    float minT = kFltMax;
    int closest = -1;
    V3 cn;
    tie = false;

    auto accept = [&](int i, float t, V3 n) {
        if (t > 0.0f)
        {
            if (fabsf(t - minT) <= 1e-5f*fabsf(t))
                tie = true;
            if (t < minT)
            {
                minT = t;
                closest = i;
                cn = n;
            }
        }
    };
    const bool finiteAll = __all(finite_bits(rcp.x) && finite_bits(rcp.y) && finite_bits(rcp.z) &&
                                 finite_bits(o.x) && finite_bits(o.y) && finite_bits(o.z));

    // the first block of opposing pairs (A0 B0 A1 B1 R - - -), unless a lane of the wave has both planes of a pair ahead
    constexpr bool kPairBlock = baked::kPlanePairEnd >= 8;
    bool paired = false;
    if constexpr (kPairBlock)
    {
        const ConstF4V e0 = baked::plane_eq<0>(), e1 = baked::plane_eq<1>(), e2 = baked::plane_eq<2>(), e3 = baked::plane_eq<3>(), e4 = baked::plane_eq<4>();
        constexpr uint32_t idr = baked::kPlaneIdx[4], ids = baked::kPlaneIdx[5];
        const PlanePair p0 = plane_pair_pick(o.x, o.y, o.z, d.x, d.y, d.z, e0.x, e0.y, e0.z, e0.w, e1.w);
        const PlanePair p1 = plane_pair_pick(o.x, o.y, o.z, d.x, d.y, d.z, e2.x, e2.y, e2.z, e2.w, e3.w);
        if (!__any(p0.both || p1.both))
        {
            paired = true;
            auto accept_of_pair = [&](const PlanePair& pp, const ConstF4V& ea, const ConstF4V& eb, int ia, int ib) {
                float t;
                if (plane_pair_hit(pp, t))
                {
                    if (fabsf(t - minT) <= 1e-5f*fabsf(t))
                        tie = true;
                    if (t < minT)
                    {
                        minT = t;
                        if (pp.b) { closest = ib; cn = V3(eb.x, eb.y, eb.z); }
                        else      { closest = ia; cn = V3(ea.x, ea.y, ea.z); }
                    }
                }
            };
            float t4;
            const bool h4 = ray_plane(o, d, e4.x, e4.y, e4.z, e4.w, t4);
            accept_of_pair(p0, e0, e1, (int)(ids & 255u), (int)((ids >> 8) & 255u));
            accept_of_pair(p1, e2, e3, (int)((ids >> 16) & 255u), (int)(ids >> 24));
            if (h4) accept((int)idr, t4, V3(e4.x, e4.y, e4.z));
        }
    }
    // the single planes: from the block's end, or the whole table slot by slot where the wave left the pairs
    if constexpr (kPairBlock)
    {
        if (paired)
            baked::single_planes<8>(o, d, accept);
        else
            baked::single_planes<0>(o, d, accept);
    }
    else
        baked::single_planes<0>(o, d, accept);

    // the primitives of the scan mask, in primitive order: box and record are constants, the kind is decided here
    baked::static_for<0, baked::kNumPrims>([&](auto ic) {
        constexpr int i = decltype(ic)::v;
        if constexpr (((baked::kScanMask >> i) & 1ull) != 0ull)
        {
            if constexpr (baked::kBoxes[i*8 + 6] == 0u)
            {
                constexpr int w = i*8;
                const float minx = baked::word_f(baked::kBoxes[w]), miny = baked::word_f(baked::kBoxes[w + 1]), minz = baked::word_f(baked::kBoxes[w + 2]),
                            maxx = baked::word_f(baked::kBoxes[w + 3]), maxy = baked::word_f(baked::kBoxes[w + 4]), maxz = baked::word_f(baked::kBoxes[w + 5]);
                float tb;
                if (!(finiteAll ? ray_aabb_minmax(o, rcp, minx, miny, minz, maxx, maxy, maxz, tb) : ray_aabb(o, rcp, minx, miny, minz, maxx, maxy, maxz, tb)))
                    return;
            }
            const Prim64 rec = baked::prim<i>();
            float t;
            V3 n;
            if (prim_intersect<SC, Stack, COUNT, false, true>(sc, i, st, 0, o, d, time, t, n, ctr, 0.0f, rcp, true, &rec))
                accept(i, t, n);
        }
    });

    outT = minT;
    outN = face_forward(cn, -d);
    return closest;
}

} // namespace tn

#endif // TN_BAKED_SCENE

// tn_query.h -- k_query: ray queries on the resident scene (tinsel_hip_trace_rays / tinsel_hip_trace_camera).
//
// The reference's Trace() (render.cpp:17-62) for rays the CALLER chooses: one ray per lane, the same trace<> the path kernels run (flat scan
// with its tie re-trace where the scene has one, the scene BVH walk elsewhere), so a record is what a path would have seen at that ray.
//   kQueryClosest   in: tinsel_ray[n]  out: tinsel_ray_hit[n]   t, primitive, FaceForward(n, -d); a miss is FLT_MAX, -1, (0, 0, 0)
//   kQueryOccluded  in: tinsel_ray[n]  out: uint32_t[n]         1 iff some primitive gives 0 < t < tmax.  The scene BVH walk and the mesh walks under
//                                                               it stop at the first such hit; the flat scan (trace<> on a flat-scan scene) never
//                                                               stops early and answers from its closest hit -- plan_query sends occlusion
//                                                               queries of such scenes to k_query_refill's walk where meshes are in HBM
//   kQueryCamera    in: the camera     out: tinsel_ray_hit[W*H] kQueryClosest on GenerateRay(i, j) of every pixel, k_normals' rays at `time`
// A ray is two 16-byte loads, a record two 16-byte stores (the occlusion word one 4-byte store), all typed as HBM (tn_walk.h's GlobalF4):
// a caller's pointer is generic to the compiler, and generic accesses are flat ones that wait on both counters.
// LDS as k_normals / k_cost: [stackEntries][kBlock] stack words, kScanWords, the staged arena (LDS: the whole scene is in it; else the bytes
// scene.arenaLdsBytes says, meshes in HBM walked inline through ray_mesh).  Nothing but `out` is written: no statistics, no path state.
#pragma once

#include "tn_path_state.h"

namespace tn {

enum QueryMode : int { kQueryClosest = 0, kQueryOccluded = 1, kQueryCamera = 2 };

struct QueryJob
{
    const void* rays;       // tinsel_ray[n] (null: kQueryCamera)
    void* out;              // tinsel_ray_hit[n] or uint32_t[n]
    uint32_t n;             // rays (kQueryCamera: width*height)
    int width;              // kQueryCamera: pixels per row
    float time;             // kQueryCamera: the pose of moving primitives
    uint32_t first;         // kQueryCamera: the pixel of record 0 (the host entry walks a frame in chunks)
    uint32_t* cursor;       // k_query_refill: the next ray nobody has claimed -- a word of this launch's own, zeroed in front of it on its stream
};

typedef __attribute__((address_space(1))) WalkF4* GlobalF4Out;
typedef __attribute__((address_space(1))) uint32_t* GlobalU32Out;

template <int MODE, bool LDS>
__global__ __launch_bounds__(kBlock, TN_WAVES_TRACE) void k_query(DevScene scIn, QueryJob job, CameraParams cam, int stackEntries)
{
    extern __shared__ uint32_t s_stack[];      // [stackEntries][kBlock], sized at launch
    LdsStack<kBlock> st = { s_stack + threadIdx.x };
    SceneT<LDS> sc;
    stage_scene_lds(sc, scIn, s_stack + stackEntries*kBlock + kScanWords);

    const uint32_t idx = blockIdx.x*kBlock + threadIdx.x;
    if (idx >= job.n)
        return;

    V3 o, d;
    float time, tmax = 0.0f;
    if (MODE == kQueryCamera)
    {
        const uint32_t pix = job.first + idx;
        const int j = (int)(pix/(uint32_t)job.width);
        const int i = (int)(pix - (uint32_t)j*(uint32_t)job.width);
        generate_ray(cam, float(i), float(j), o, d);
        time = job.time;
    }
    else
    {
        GlobalF4 rp = as_global(job.rays) + (size_t)idx*2;
        const WalkF4 a = rp[0], b = rp[1];
        o = V3(a.x, a.y, a.z);
        time = a.w;
        d = V3(b.x, b.y, b.z);
        tmax = b.w;
    }

    float t;
    V3 n;
    TraceCounters ctr = { 0, 0, 0 };
    if (MODE == kQueryOccluded)
    {
        // (a stopped trace's t is SOME hit's, below tmax; one that ran to its end has the closest: `t < tmax` says the same of both.
        // NaN and non-positive tmax: no t > 0 is below it, the walk never stops early and the answer is 0)
        const int prim = trace<SceneT<LDS>, LdsStack<kBlock>, false, true>(sc, st, o, d, time, t, n, ctr, tmax);
        ((GlobalU32Out)(uintptr_t)job.out)[idx] = (prim >= 0 && t < tmax) ? 1u : 0u;
    }
    else
    {
        const int prim = trace<SceneT<LDS>, LdsStack<kBlock>, false>(sc, st, o, d, time, t, n, ctr);
        WalkF4 ra, rb;
        ra.x = prim >= 0 ? t : kFltMax;
        ra.y = __int_as_float(prim >= 0 ? prim : -1);
        ra.z = prim >= 0 ? n.x : 0.0f;
        ra.w = prim >= 0 ? n.y : 0.0f;
        rb.x = prim >= 0 ? n.z : 0.0f;
        rb.y = 0.0f; rb.z = 0.0f; rb.w = 0.0f;
        GlobalF4Out op = (GlobalF4Out)(uintptr_t)job.out + (size_t)idx*2;
        op[0] = ra;
        op[1] = rb;
    }
}

// ---------------------------------------------------------------------------
// k_query_refill: the same queries with RAY REPLACEMENT.  Persistent workgroups; a lane whose ray is finished takes the next one, so a wave
// is not as slow as its slowest ray.  Rays come from an LDS range {next, end} per workgroup (one 64-bit word, claimed by a wave's first lane
// with one LDS compare-and-swap for all its idle lanes), fed kQueryRefillChunk rays at a time by ONE global atomic on job.cursor -- no atomic
// per ray.  Closest and occluded only (a camera frame's rays are coherent: k_query).  Every lane runs the scene BVH walk of trace<> (the oracle's order, never the flat scan: the scan is wave-uniform and has no
// place to refill) one stack entry per turn; a leaf's primitive test, a mesh walk included, is one turn.
constexpr uint32_t kQueryRefillChunk = 2048;
constexpr int kQueryRefillMin = 16;         // idle lanes that trigger a refill

template <int MODE, bool LDS>
__global__ __launch_bounds__(kBlock, TN_WAVES_TRACE) void k_query_refill(DevScene scIn, QueryJob job, CameraParams, int stackEntries)
{
    extern __shared__ uint32_t s_stack[];      // [stackEntries][kBlock], then: {next, end} (64 bits), lock, done
    LdsStack<kBlock> st = { s_stack + threadIdx.x };
    uint32_t* const ctl = s_stack + stackEntries*kBlock;
    if (threadIdx.x == 0)
    {
        ctl[0] = 0u; ctl[1] = 0u; ctl[2] = 0u; ctl[3] = 0u;
    }
    SceneT<LDS> sc;
    stage_scene_lds(sc, scIn, s_stack + stackEntries*kBlock + kScanWords);
    __syncthreads();
    unsigned long long* const range = reinterpret_cast<unsigned long long*>(ctl);
    volatile uint32_t* const vctl = ctl;

    const int lane = lane_id();
    constexpr bool ANY = MODE == kQueryOccluded;
    bool active = false, dry = false;
    uint32_t idx = 0;
    V3 o, d, rcp, cn;
    float time = 0.0f, tmax = 0.0f, minT = kFltMax;
    int closest = -1, sp = 0;
    TraceCounters ctr = { 0, 0, 0 };

    for (;;)
    {
        const unsigned long long idleMask = __ballot(!active);
        const int idle = __popcll(idleMask);
        if (!dry && (idle >= kQueryRefillMin || idle == kWave))
        {
            uint32_t base = 0, got = 0;
            if (lane == 0)
            {
                // (ends: a claim succeeds, or nothing is left; the lock's holder never waits for anyone, so a waiting wave always gets on)
                for (;;)
                {
                    const unsigned long long v = *reinterpret_cast<volatile unsigned long long*>(range);
                    const uint32_t cur = (uint32_t)v, end = (uint32_t)(v >> 32);
                    if (cur < end)
                    {
                        const uint32_t take = min((uint32_t)idle, end - cur);
                        if (atomicCAS(range, v, ((unsigned long long)end << 32) | (cur + take)) == v)
                        {
                            base = cur; got = take;
                            break;
                        }
                        continue;
                    }
                    if (vctl[3])
                        break;              // nothing left anywhere
                    if (atomicCAS(ctl + 2, 0u, 1u) == 0u)
                    {
                        // this wave refills the workgroup's range (still empty? another wave may just have done it)
                        const unsigned long long v2 = *reinterpret_cast<volatile unsigned long long*>(range);
                        if ((uint32_t)v2 >= (uint32_t)(v2 >> 32) && !vctl[3])
                        {
                            const uint32_t g = atomicAdd(job.cursor, kQueryRefillChunk);
                            if (g >= job.n)
                                atomicExch(ctl + 3, 1u);
                            else
                                atomicExch(range, ((unsigned long long)min(g + kQueryRefillChunk, job.n) << 32) | g);
                        }
                        __threadfence_block();
                        atomicExch(ctl + 2, 0u);
                    }
                    else
                        __builtin_amdgcn_s_sleep(4);
                }
            }
            base = (uint32_t)__shfl((int)base, 0);
            got = (uint32_t)__shfl((int)got, 0);
            if (got == 0)
                dry = true;
            const uint32_t rank = (uint32_t)__popcll(idleMask & ((1ull << lane) - 1ull));
            if (!active && rank < got)
            {
                idx = base + rank;
                GlobalF4 rp = as_global(job.rays) + (size_t)idx*2;
                const WalkF4 a = rp[0], b = rp[1];
                o = V3(a.x, a.y, a.z);
                time = a.w;
                d = V3(b.x, b.y, b.z);
                tmax = b.w;
                rcp = rcp3_cr(d);
                minT = kFltMax;
                closest = -1;
                sp = 0;
                st.set(sp++, sc.root);
                active = true;
            }
        }
        if (__ballot(active) == 0ull)
        {
            if (dry)
                break;
            continue;
        }
        if (active)
        {
            const uint32_t ref = st.get(--sp);
            if (ref & kLeafBit)
            {
                float t;
                V3 n;
                const int index = (int)(ref & ~kLeafBit);
                if (prim_intersect<SceneT<LDS>, LdsStack<kBlock>, false, ANY>(sc, index, st, sp, o, d, time, t, n, ctr, tmax, rcp, true))
                {
                    if (t < minT && t > 0.0f)
                    {
                        minT = t;
                        closest = index;
                        cn = n;
                        if (ANY && t < tmax)
                            sp = 0;
                    }
                }
            }
            else
            {
                const Node64 nd = load_node(sc.nodes, ref);
                float tL, tR;
                const bool hL = ray_aabb(o, rcp, nd.lminx, nd.lminy, nd.lminz, nd.lmaxx, nd.lmaxy, nd.lmaxz, tL);
                const bool hR = ray_aabb(o, rcp, nd.rminx, nd.rminy, nd.rminz, nd.rmaxx, nd.rmaxy, nd.rmaxz, tR);
                uint32_t first = nd.left, second = nd.right;
                if (hL && hR && (tL < tR))
                {
                    first = nd.right;
                    second = nd.left;
                }
                if (hL)
                    st.set(sp++, first);
                if (hR)
                    st.set(sp++, second);
            }
            if (sp == 0)
            {
                if (ANY)
                    ((GlobalU32Out)(uintptr_t)job.out)[idx] = (closest >= 0 && minT < tmax) ? 1u : 0u;
                else
                {
                    const V3 n = face_forward(cn, -d);
                    WalkF4 ra, rb;
                    ra.x = closest >= 0 ? minT : kFltMax;
                    ra.y = __int_as_float(closest);
                    ra.z = closest >= 0 ? n.x : 0.0f;
                    ra.w = closest >= 0 ? n.y : 0.0f;
                    rb.x = closest >= 0 ? n.z : 0.0f;
                    rb.y = 0.0f; rb.z = 0.0f; rb.w = 0.0f;
                    GlobalF4Out op = (GlobalF4Out)(uintptr_t)job.out + (size_t)idx*2;
                    op[0] = ra;
                    op[1] = rb;
                }
                active = false;
            }
        }
    }
}

} // namespace tn

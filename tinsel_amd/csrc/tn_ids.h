// tn_ids.h -- ID mattes (tinsel_hip_render_id_mattes*): per pixel a ranked list of (primitive id, filter-weight sum) pairs on the beauty's
// own samples -- k_ids, k_ids_accumulate (tiled and generic), k_ids_rank.
//
// An id does not average, so it cannot go through the float4 accumulate kernels.  k_ids is k_features with a 4-byte record: one lane per
// path slot, camera_sample as begin_path runs it, one closest-hit trace<>, and the primitive's index (kIdMiss where the path left the
// scene) by slot.  k_ids_accumulate is AddSample's visiting order (tn_accumulate.h: passes ascending, generating pixels in raster order) as
// an order-preserving gather of LISTS: a pixel's thread holds kIdMaxSlots (id, weight) pairs, the residual and the total in registers --
// loaded from the call's per-pixel state at the start of a batch, stored at its end, so slots keep first-seen order from batch to batch --
// and per candidate that covers the pixel with weight w:
//     total += w;  a slot that holds the id: weight += w;  else the first empty slot (of the `slots` in use): (id, w);  else residual += w.
// A candidate with w == +0 claims no slot; its adds of +0 to sums that are never negative change no bit, so they are left to happen.
// The slot search is a compare / select chain unrolled over the eight slots with constant indices: no register array is indexed by a
// run-time value (that would go to scratch), no atomic, and a wave diverges only at the covers test the accumulate kernels have.
// k_ids_rank sorts a pixel's eight pairs with a fixed compare-exchange network -- weight descending, ties by ascending id, empty slots
// (weight 0, kIdEmpty) last -- and writes the caller's planar buffers.
// The state is planar, pixel-major inside a plane: ids[kIdMaxSlots][W*H], weights[kIdMaxSlots + 2][W*H] (then residual, total), so a wave's
// load or store of a plane is one run.  Every float operation is one fp32 add, or AddSample's one multiply of the two separable weights.
#pragma once

#include "tn_accumulate.h"
#include "tn_features.h"

namespace tn {

constexpr int kIdMiss = -1;             // TINSEL_ID_MISS
constexpr int kIdEmpty = -2;            // TINSEL_ID_EMPTY
constexpr int kIdMaxSlots = 8;          // TINSEL_ID_MAX_SLOTS

// (k_ids takes k_features' job and launch arguments: FeatureJob::out is int32[batch slots], the id of every path by slot; planeStride and
// mask are not read)
typedef __attribute__((address_space(1))) int* GlobalI32Out;

template <bool LDS>
__global__ __launch_bounds__(kBlock, TN_WAVES_TRACE) void k_ids(DevScene scIn, FeatureJob job, CameraParams cam, FrameParams fp,
                                                                const uint32_t* __restrict__ passSeeds, int stackEntries)
{
    extern __shared__ uint32_t s_stack[];      // [stackEntries][kBlock], sized at launch
    LdsStack<kBlock> st = { s_stack + threadIdx.x };
    SceneT<LDS> sc;
    stage_scene_lds(sc, scIn, s_stack + stackEntries*kBlock + kScanWords);

    const uint32_t idx = blockIdx.x*kBlock + threadIdx.x;
    int s = 0, i = 0, j = 0;
    if (!(idx < fp.genCount && slot_pixel(fp, idx, s, i, j)))
        return;

    Rng rng;
    float rx, ry, time;
    V3 o, d;
    camera_sample(cam, fp, i, j, passSeeds[fp.passBase + s], rng, rx, ry, time, o, d);

    float t;
    V3 n;
    TraceCounters ctr = { 0, 0, 0 };
    const int prim = trace<SceneT<LDS>, LdsStack<kBlock>, false>(sc, st, o, d, time, t, n, ctr);
    ((GlobalI32Out)(uintptr_t)job.out)[idx] = prim >= 0 ? prim : kIdMiss;
}

// A pixel's list in registers.  Every loop below is unrolled over constant indices.
struct IdList
{
    int id[kIdMaxSlots];
    float w[kIdMaxSlots];
    float residual, total;

    TN_D void load(const int* __restrict__ ids, const float* __restrict__ weights, size_t npix, size_t pix)
    {
#pragma unroll
        for (int k = 0; k < kIdMaxSlots; ++k)
        {
            id[k] = ids[(size_t)k*npix + pix];
            w[k] = weights[(size_t)k*npix + pix];
        }
        residual = weights[(size_t)kIdMaxSlots*npix + pix];
        total = weights[(size_t)(kIdMaxSlots + 1)*npix + pix];
    }
    TN_D void store(int* __restrict__ ids, float* __restrict__ weights, size_t npix, size_t pix) const
    {
#pragma unroll
        for (int k = 0; k < kIdMaxSlots; ++k)
        {
            ids[(size_t)k*npix + pix] = id[k];
            weights[(size_t)k*npix + pix] = w[k];
        }
        weights[(size_t)kIdMaxSlots*npix + pix] = residual;
        weights[(size_t)(kIdMaxSlots + 1)*npix + pix] = total;
    }
    // one candidate that covers the pixel: id `c`, weight `wt` >= +0, `slots` of the eight in use
    TN_D void add(int c, float wt, int slots)
    {
        total += wt;
        bool placed = false;
#pragma unroll
        for (int k = 0; k < kIdMaxSlots; ++k)
        {
            const bool m = id[k] == c;          // (an id is never kIdEmpty, and a list holds an id once)
            w[k] = m ? w[k] + wt : w[k];
            placed = placed || m;
        }
        placed = placed || !(wt > 0.0f);        // weight +0: no slot; the add to the residual below is of +0
#pragma unroll
        for (int k = 0; k < kIdMaxSlots; ++k)
        {
            const bool e = !placed && k < slots && id[k] == kIdEmpty;
            id[k] = e ? c : id[k];
            w[k] = e ? wt : w[k];
            placed = placed || e;
        }
        residual = placed ? residual : residual + wt;
    }
};

// Generic form, any filter: one thread per pixel, k_accumulate's loops
__global__ __launch_bounds__(kBlock, 4) void k_ids_accumulate(const int* __restrict__ rec, FrameParams fp, int* __restrict__ ids, float* __restrict__ weights,
                                                              const uint32_t* __restrict__ passSeeds, int slots)
{
    const int npix = fp.width*fp.height;
    const int pix = blockIdx.x*kBlock + threadIdx.x;
    if (pix >= npix)
        return;
    const int py = pix/fp.width;
    const int px = pix - py*fp.width;

    const float fw = fp.filterWidth;
    const int reachLo = 1 + (int)floorf(fw);
    const int reachHi = (int)ceilf(fw);
    const int i0 = maxI(0, px - reachLo), i1 = minI(fp.width - 1, px + reachHi);
    const int j0 = maxI(0, py - reachLo), j1 = minI(fp.height - 1, py + reachHi);

    IdList L;
    L.load(ids, weights, (size_t)npix, (size_t)pix);

    for (int s = fp.accBegin; s < fp.accEnd; ++s)
    {
        for (int j = j0; j <= j1; ++j)
        {
            for (int i = i0; i <= i1; ++i)
            {
                if (!pixel_owned(fp, i, j))
                    continue;       // path not generated by this shard
                float rx, ry;
                raster_position(fp, passSeeds, s, i, j, rx, ry);
                if (!splat_footprint(fp, rx, ry).covers(px, py))
                    continue;
                const int c = rec[slot_of(fp, s, i, j)];
                const float w = fp.filterType == 0 ? 1.0f :
                                filter_gauss(px - rx, fp.filterFalloff, fp.filterOffset)*filter_gauss(py - ry, fp.filterFalloff, fp.filterOffset);
                L.add(c, w, slots);
            }
        }
    }

    L.store(ids, weights, (size_t)npix, (size_t)pix);
}

// Tiled form, filter widths up to 2: one 16 x 16 pixel tile per workgroup (tile_geometry; a shard: the tiles of its list).  Per pass the
// (16 + halo)^2 candidates of the tile are staged into LDS once -- id, column run, row run (pack_run) and the separable weights of the
// footprint's columns and rows (stage_weights) -- and every pixel walks its window of them in raster order.  Candidates outside the frame
// or of another shard are staged as "covers nothing".  The next pass's ids are requested before the current pass is gathered.
// SPAN = the window's edge as a compile-time constant (3, 4: filter widths up to 1), 0 = the window's bounds at run time.
template <int SPAN>
__global__ __launch_bounds__(kBlock, 4) void k_ids_accumulate_tiled(const int* __restrict__ rec, FrameParams fp, int* __restrict__ ids, float* __restrict__ weights,
                                                                    const uint32_t* __restrict__ passSeeds, const int* __restrict__ tileList, int slots)
{
    constexpr int kSide = SPAN > 0 ? kAccTile + SPAN - 1 : kAccSide;
    constexpr int kEntries = kSide*kSide;
    constexpr int kFoot = (SPAN > 0 ? 3 : kAccMaxFoot) + 1;         // (+ 1: the row / column a rounded-up r + fw adds, k_accumulate_tiled)
    constexpr int kEnt = (kEntries + kBlock - 1)/kBlock;
    __shared__ int s_id[kEntries];
    __shared__ uint32_t s_x[kEntries];                  // pack_run(startX, nX); nX == 0: covers nothing
    __shared__ uint32_t s_y[kEntries];                  // pack_run(startY, nY)
    __shared__ float s_wx[kFoot][kEntries];
    __shared__ float s_wy[kFoot][kEntries];
    __shared__ unsigned long long s_exp[32];            // expf's table
    if (threadIdx.x < 32)
        s_exp[threadIdx.x] = kExp2fTab[threadIdx.x];
    __syncthreads();

    const AccTile g = tile_geometry(fp, tileList);
    const int side = g.side;

    // the (at most two) candidate entries this thread stages every pass
    int le[kEnt], gx[kEnt], gy[kEnt], nextId[kEnt];
    bool stage[kEnt], live[kEnt];
#pragma unroll
    for (int k = 0; k < kEnt; ++k)
    {
        const int e = threadIdx.x + k*kBlock;
        const int ex = e % side, ey = e/side;
        gx[k] = g.ox + ex; gy[k] = g.oy + ey;
        le[k] = ey*kSide + ex;
        stage[k] = e < side*side;
        live[k] = stage[k] && candidate_live(fp, gx[k], gy[k]);
        nextId[k] = kIdMiss;
    }
    auto request = [&](int s) {
        if (s < fp.accEnd)
#pragma unroll
            for (int k = 0; k < kEnt; ++k)
                if (live[k])
                    nextId[k] = rec[slot_of(fp, s, gx[k], gy[k])];
    };
    request(fp.accBegin);

    const int lx = threadIdx.x % kAccTile, ly = threadIdx.x/kAccTile;
    const int px = g.tx*kAccTile + lx, py = g.ty*kAccTile + ly;
    const bool inside = px < fp.width && py < fp.height;
    const size_t npix = (size_t)fp.width*fp.height, pix = (size_t)py*fp.width + px;

    IdList L;
#pragma unroll
    for (int k = 0; k < kIdMaxSlots; ++k)
    {
        L.id[k] = kIdEmpty;
        L.w[k] = 0.0f;
    }
    L.residual = 0.0f; L.total = 0.0f;
    if (inside)
        L.load(ids, weights, npix, pix);

    // this pixel's candidate window, in LDS coordinates (clipped to the frame like the reference's loops)
    const int i0 = maxI(0, px - g.reachLo) - g.ox, i1 = minI(fp.width - 1, px + g.reachHi) - g.ox;
    const int j0 = maxI(0, py - g.reachLo) - g.oy, j1 = minI(fp.height - 1, py + g.reachHi) - g.oy;

    auto add = [&](int e) {
        const uint32_t xm = s_x[e], ym = s_y[e];
        const uint32_t kx = (uint32_t)(px - (int)(xm & 0xffffu)), ky = (uint32_t)(py - (int)(ym & 0xffffu));
        if (kx >= (xm >> 16) || ky >= (ym >> 16))
            return;
        L.add(s_id[e], g.gauss ? s_wx[kx][e]*s_wy[ky][e] : 1.0f, slots);
    };

    for (int s = fp.accBegin; s < fp.accEnd; ++s)
    {
        int curId[kEnt];
#pragma unroll
        for (int k = 0; k < kEnt; ++k)
            curId[k] = nextId[k];
        request(s + 1);

#pragma unroll
        for (int k = 0; k < kEnt; ++k)
        {
            if (!stage[k])
                continue;
            uint32_t xm = 0u, ym = 0u;
            if (live[k])
            {
                Candidate q;
                raster_position(fp, passSeeds, s, gx[k], gy[k], q.rx, q.ry);
                q.f = splat_footprint(fp, q.rx, q.ry);
                xm = pack_run(q.f.startX, q.f.nX);
                ym = q.rows();
                if (g.gauss)
                    stage_weights(fp, q, s_wx, s_wy, le[k], s_exp);
            }
            s_id[le[k]] = curId[k];
            s_x[le[k]] = xm;
            s_y[le[k]] = ym;
        }
        __syncthreads();

        if (inside)
        {
            if (SPAN > 0)
            {
                // the window of pixel (lx, ly) starts at LDS entry (lx, ly): px - reachLo - ox == lx
#pragma unroll
                for (int dj = 0; dj < SPAN; ++dj)
#pragma unroll
                    for (int di = 0; di < SPAN; ++di)
                        add((ly + dj)*kSide + lx + di);
            }
            else
            {
                for (int j = j0; j <= j1; ++j)
                    for (int i = i0; i <= i1; ++i)
                        add(j*kSide + i);
            }
        }
        __syncthreads();
    }

    if (inside)
        L.store(ids, weights, npix, pix);
}

// The ranking and the caller's layout: out_ids[slots][W*H], out_weights[slots + 2][W*H] (planes `slots` and `slots + 1`: residual, total)
TN_D void rank_exchange(int& ia, float& wa, int& ib, float& wb)
{
    // b in front of a: the heavier one, of two equal weights the smaller id
    const bool swap = wb > wa || (wb == wa && ib < ia);
    const int ti = swap ? ib : ia;
    const float tw = swap ? wb : wa;
    ib = swap ? ia : ib; wb = swap ? wa : wb;
    ia = ti; wa = tw;
}

__global__ __launch_bounds__(kBlock) void k_ids_rank(const int* __restrict__ ids, const float* __restrict__ weights, int npixIn, int slots,
                                                     int* __restrict__ outIds, float* __restrict__ outWeights)
{
    const size_t npix = (size_t)npixIn;
    const size_t pix = (size_t)blockIdx.x*kBlock + threadIdx.x;
    if (pix >= npix)
        return;
    IdList L;
    L.load(ids, weights, npix, pix);
    // Batcher's odd-even merge sort of eight: 19 compare-exchanges
#define TN_CX(A, B) rank_exchange(L.id[A], L.w[A], L.id[B], L.w[B])
    TN_CX(0, 1); TN_CX(2, 3); TN_CX(4, 5); TN_CX(6, 7);
    TN_CX(0, 2); TN_CX(1, 3); TN_CX(4, 6); TN_CX(5, 7);
    TN_CX(1, 2); TN_CX(5, 6);
    TN_CX(0, 4); TN_CX(1, 5); TN_CX(2, 6); TN_CX(3, 7);
    TN_CX(2, 4); TN_CX(3, 5);
    TN_CX(1, 2); TN_CX(3, 4); TN_CX(5, 6);
#undef TN_CX
#pragma unroll
    for (int k = 0; k < kIdMaxSlots; ++k)
        if (k < slots)
        {
            outIds[(size_t)k*npix + pix] = L.id[k];
            outWeights[(size_t)k*npix + pix] = L.w[k];
        }
    outWeights[(size_t)slots*npix + pix] = L.residual;
    outWeights[(size_t)(slots + 1)*npix + pix] = L.total;
}

} // namespace tn

// tn_samples.h -- sample maps (tinsel_hip_render_sample_map*): a per-pixel pass count in one call.
//
// Pixel q of the frame gets the samples of levels 0 .. counts[q] - 1; level t is the path a render starts for q in pass pass_begin + t.  A
// batch holds a run of consecutive levels [t0, t0 + L); the host's exclusive prefix sum off[0 .. W*H] over clamp(counts[q] - t0, 0, L)
// makes the slot space COMPACT: the slot of (q, t) is off[q] + (t - t0), off[W*H] paths in all.  The layout is pixel-major -- a pixel's
// levels side by side, then the next pixel's -- because both kernels then touch one short run of `off` and of the radiance per pixel: the
// accumulate keeps a candidate's off and count in registers for the whole tile and walks rad[off + t] level by level, and a wave of the
// generation kernel, 64 consecutive slots, spans few pixels.  (Level-major would need one offset table per level.)
//
// k_generate_samples is the fifth generation kernel beside k_generate, k_generate_rays, k_generate_gather and k_generate_views: a fifth source
// of paths for generate_regions (tn_split.h).  Generation index idx belongs to the pixel q with off[q] <= idx < off[q + 1] -- an upper-bound
// search -- and is level idx - off[q] of it; the path is begin_path -- unchanged -- on the slot a render's batch of those levels gives
// (level, q), and its own slot is idx.  The search: per 64 indices the WAVE finds the pixels of its first and of its last live index, each
// by galloping forward from the one found before (the wave's indices only grow, so in the steady state that is a probe or two, read through
// the scalar cache), and every lane then bisects between the two, a handful of pixels.  A plain walk forward from the first lane's pixel
// was not kept: a crop or a sparse map puts runs of thousands of empty pixels between two live ones and the walk crosses them one load at a
// time; a per-lane bisection of the whole table is 18 dependent loads a path at 512 x 512 where this form makes 1 + log2(pixels a wave spans).
//
// k_samples_accumulate is k_views_accumulate's gather with a level loop that knows which candidates exist: a staged entry keeps its off and
// its count in the batch in registers, at level t it fetches rad[off + t] if t < count and is staged as "covers nothing" otherwise -- NOT as
// a black sample, the weight channel must not see it --, and the loop of a block runs to the largest count among the tile's candidates (one
// LDS maximum, block-uniform, so the barriers stay legal).  A tile none of whose candidates has a sample in the batch returns before it
// loads its pixels.  Built from the accumulate kernels' own device functions: the same adds in the same order.  (Named k_samples_accumulate,
// not k_accumulate_samples: the resource tests pin the set of kernels whose name begins with k_accumulate.)
#pragma once

#include "tn_split.h"
#include "tn_accumulate.h"

namespace tn {

struct SamplesJob
{
    const uint32_t* off;    // [npix + 1]: exclusive prefix sum of the pixels' counts in the batch
    uint32_t npix;          // W*H
    uint32_t count;         // paths of the batch: off[npix]
};

// The largest q in [lo, n) with off[q] <= idx, for off[lo] <= idx (else the search starts over at 0; off[0] == 0): doubling steps
// forward, then a bisection of the last step
TN_D uint32_t samples_pixel_from(const uint32_t* __restrict__ off, uint32_t lo, uint32_t n, uint32_t idx)
{
    if (off[lo] > idx)
        lo = 0u;
    uint32_t hi = n - 1u;
    for (uint32_t step = 1u; ; step <<= 1)
    {
        const uint32_t probe = lo + step;
        if (probe >= n)
            break;
        if (off[probe] > idx)
        {
            hi = probe - 1u;
            break;
        }
        lo = probe;
    }
    while (lo < hi)
    {
        const uint32_t mid = lo + (hi - lo + 1u)/2u;
        if (off[mid] <= idx)
            lo = mid;
        else
            hi = mid - 1u;
    }
    return lo;
}

__global__ __launch_bounds__(kBlock, 4) void k_generate_samples(SplitState ss, QueueCtl q, SamplesJob job, CameraParams cam, FrameParams fp,
                                                             const uint32_t* __restrict__ passSeeds, const PrimBox* __restrict__ primBoxes, BinPrims bp)
{
    uint32_t hint = 0u;         // the pixel of the last index this wave placed (wave-uniform)
    generate_regions(ss, q, job.count, primBoxes, bp, [&](uint32_t idx, PathRegs& p, uint32_t&) -> bool {
        // (the lanes that come here are the wave's first n: their indices are first .. first + n - 1)
        const uint32_t first = __builtin_amdgcn_readfirstlane(idx);
        const uint32_t last = first + (uint32_t)__popcll(__ballot(1)) - 1u;
        const uint32_t qLo = __builtin_amdgcn_readfirstlane(samples_pixel_from(job.off, hint, job.npix, first));
        const uint32_t qHi = __builtin_amdgcn_readfirstlane(samples_pixel_from(job.off, qLo, job.npix, last));
        hint = qHi;
        uint32_t lo = qLo, hi = qHi;
        while (lo < hi)
        {
            const uint32_t mid = lo + (hi - lo + 1u)/2u;
            if (job.off[mid] <= idx)
                lo = mid;
            else
                hi = mid - 1u;
        }
        // (pixels without a sample in the batch have off[q] == off[q + 1] and are never the LARGEST q at or below idx)
        const uint32_t level = idx - job.off[lo];
        float rx, ry;
        // (one shard, so every slot has a pixel: begin_path does not refuse)
        return begin_path(cam, fp, passSeeds, level*job.npix + lo, p, rx, ry);
    });
}

// SPAN as k_accumulate_tiled's: the candidate window's edge at compile time (3, 4), or 0 for the window's bounds at run time (widths up to 2)
template <int SPAN>
__global__ __launch_bounds__(kBlock, 4) void k_samples_accumulate(PathState ps, FrameParams fp, float4* __restrict__ accum, const uint32_t* __restrict__ passSeeds,
                                                               const uint32_t* __restrict__ off)
{
    constexpr int kSide = SPAN > 0 ? kAccTile + SPAN - 1 : kAccSide;
    constexpr int kEntries = kSide*kSide;
    constexpr int kFoot = (SPAN > 0 ? 3 : kAccMaxFoot) + 1;         // (+ 1: the row / column a rounded-up r + fw adds, k_accumulate_tiled)
    constexpr int kEnt = (kEntries + kBlock - 1)/kBlock;
    __shared__ float4 s_c[kEntries];                 // Candidate::record()
    __shared__ uint32_t s_y[kEntries];               // Candidate::rows()
    __shared__ float s_wx[kFoot][kEntries];
    __shared__ float s_wy[kFoot][kEntries];
    __shared__ unsigned long long s_exp[32];
    __shared__ uint32_t s_levels;                    // the largest count in the batch among this tile's candidates
    if (threadIdx.x < 32)
        s_exp[threadIdx.x] = kExp2fTab[threadIdx.x];
    if (threadIdx.x == 0)
        s_levels = 0u;
    __syncthreads();

    const AccTile g = tile_geometry(fp, nullptr);
    const int side = g.side, reachLo = g.reachLo;

    // the (at most two) candidate entries this thread stages every level: entry t, t + 256 -- where its pixel's samples start in the
    // batch's radiance and how many there are, loaded once
    AccEntries<kEnt> ent;
    bool entStage[kEnt];
    uint32_t entOff[kEnt], entCount[kEnt];
    uint32_t most = 0u;
#pragma unroll
    for (int k = 0; k < kEnt; ++k)
    {
        const int e = threadIdx.x + k*kBlock;
        const int ex = e % side, ey = e/side;
        ent.gx[k] = g.ox + ex; ent.gy[k] = g.oy + ey;
        ent.le[k] = ey*kSide + ex;
        ent.live[k] = e < side*side && candidate_live(fp, ent.gx[k], ent.gy[k]);
        entStage[k] = e < side*side;                    // (entries outside the frame are staged as "covers nothing", every level)
        entOff[k] = 0u; entCount[k] = 0u;
        if (ent.live[k])
        {
            const uint32_t pix = (uint32_t)ent.gy[k]*(uint32_t)fp.width + (uint32_t)ent.gx[k];
            entOff[k] = off[pix];
            entCount[k] = off[pix + 1u] - entOff[k];
        }
        most = most > entCount[k] ? most : entCount[k];
    }
    for (int o = 32; o > 0; o >>= 1)
    {
        const uint32_t other = (uint32_t)__shfl_down((int)most, o);
        most = most > other ? most : other;
    }
    if ((threadIdx.x & 63) == 0 && most)
        atomicMax(&s_levels, most);
    __syncthreads();
    // (a batch holds fp.numPasses levels, so no count is larger)
    const int levels = minI((int)__builtin_amdgcn_readfirstlane(s_levels), fp.accEnd);
    if (levels <= 0)
        return;                                         // nothing in this batch reaches the tile: its pixels are left alone

    // level s of the entries that have one, requested a level ahead of its use (as AccEntries::request, on the compact slots)
    auto request = [&](int s) {
#pragma unroll
        for (int k = 0; k < kEnt; ++k)
            if (ent.live[k] && (uint32_t)s < entCount[k])
                ent.nextRa[k] = ps.rad[entOff[k] + (uint32_t)s];
    };
    request(0);

    const int lx = threadIdx.x % kAccTile, ly = threadIdx.x/kAccTile;
    const int px = g.tx*kAccTile + lx, py = g.ty*kAccTile + ly;
    const bool inside = px < fp.width && py < fp.height;

    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (inside)
        acc = accum[py*fp.width + px];

    // this pixel's candidate window, in LDS coordinates (clipped to the frame like the reference's loops)
    const int i0 = maxI(0, px - reachLo) - g.ox, i1 = minI(fp.width - 1, px + g.reachHi) - g.ox;
    const int j0 = maxI(0, py - reachLo) - g.oy, j1 = minI(fp.height - 1, py + g.reachHi) - g.oy;

    for (int s = 0; s < levels; ++s)
    {
        float4 curRa[kEnt];
#pragma unroll
        for (int k = 0; k < kEnt; ++k)
            curRa[k] = ent.nextRa[k];
        if (s + 1 < levels)
            request(s + 1);

#pragma unroll
        for (int k = 0; k < kEnt; ++k)
        {
            if (!entStage[k])
                continue;
            const int le = ent.le[k];
            float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);     // nX == 0: covers nothing -- also a pixel that has no sample at this level
            uint32_t ym = 0;
            if (ent.live[k] && (uint32_t)s < entCount[k])
            {
                const Candidate q = candidate_of_pass(fp, passSeeds, s, ent.gx[k], ent.gy[k], curRa[k]);
                c = q.record();
                ym = q.rows();
                if (g.gauss)
                    stage_weights(fp, q, s_wx, s_wy, le, s_exp);
            }
            s_c[le] = c;
            s_y[le] = ym;
        }
        __syncthreads();

        auto add = [&](int le) { add_candidate(acc, px, py, g.gauss, s_c, s_y, s_wx, s_wy, le); };
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
        accum[py*fp.width + px] = acc;
}

} // namespace tn

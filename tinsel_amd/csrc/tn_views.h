// tn_views.h -- view batches (tinsel_hip_render_views*): many cameras' frames of one resident scene in one call.
//
// k_generate_views is the fourth generation kernel beside k_generate (one camera's paths), k_generate_rays and k_generate_gather: a fourth
// source of paths for generate_regions (tn_split.h).  A batch holds `views` consecutive cameras times the batch's passes; generation index
// idx is path `idx % perView` of view `idx / perView`, perView = passes of the batch x W*H, and that path is begin_path -- unchanged -- of
// the view's camera on the view-local slot: the same pixel, pass seed, draws and ray a render of that camera alone starts slot
// `idx % perView` with.  The path's slot is idx, so the batch's radiance is [view][pass][pixel] and each view's part looks to an accumulate
// kernel exactly like a render's batch.  Everything downstream -- k_extend .. k_shade, k_walk, k_step -- reads buffer 0 of the dense state
// as it does after k_generate.
//
// The cameras come from a device table the host builds with make_camera (21 floats a view, padded to 96 bytes).  A wave straddles two views
// only at a view boundary, but the compiler cannot know: the record is read per lane, six 16-byte loads of one address for most waves --
// one cache line, once per 64 paths.
//
// k_views_accumulate is k_accumulate_tiled's full window (256 threads, the compile-time windows 3 and 4 and the run-time one) with a second
// grid dimension: block (t, v) adds view v's radiance, rad + v*perView, to plane v, accum + v*W*H.  It is built from the accumulate kernels'
// own device functions and makes the same adds in the same order; a batch of V views is ONE launch of V x tiles blocks where V launches of
// the existing kernels are V drains of a few tiles each.  (Named k_views_accumulate, not k_accumulate_views: the resource tests pin the
// set of kernels whose name begins with k_accumulate.)
#pragma once

#include "tn_split.h"
#include "tn_accumulate.h"

namespace tn {

// a view's camera in the device table: CameraParams (84 bytes) padded to six 16-byte loads
struct alignas(16) ViewCamera
{
    CameraParams cam;
    float pad[3];
};
static_assert(sizeof(ViewCamera) == 96, "k_generate_views reads a view's camera as six 16-byte loads");

struct ViewsJob
{
    const ViewCamera* cameras;  // the batch's first view
    uint32_t perView;           // path slots of one view in the batch: its passes x W*H
    uint32_t perViewM;          // floor((2^32 - 1)/perView): div_magic's reciprocal
    uint32_t count;             // paths of the batch: views x perView
};

__global__ __launch_bounds__(kBlock, 4) void k_generate_views(SplitState ss, QueueCtl q, ViewsJob job, FrameParams fp, const uint32_t* __restrict__ passSeeds,
                                                           const PrimBox* __restrict__ primBoxes, BinPrims bp)
{
    generate_regions(ss, q, job.count, primBoxes, bp, [&](uint32_t idx, PathRegs& p, uint32_t&) -> bool {
        uint32_t view, local;
        div_magic(idx, job.perView, job.perViewM, view, local);
        const CameraParams cam = job.cameras[view].cam;
        float rx, ry;
        // (one shard, so every slot of a view has a pixel: begin_path does not refuse)
        return begin_path(cam, fp, passSeeds, local, p, rx, ry);
    });
}

// SPAN as k_accumulate_tiled's: the candidate window's edge at compile time (3, 4), or 0 for the window's bounds at run time (widths up to 2)
template <int SPAN>
__global__ __launch_bounds__(kBlock, 4) void k_views_accumulate(PathState ps, FrameParams fp, float4* __restrict__ accum, const uint32_t* __restrict__ passSeeds,
                                                             uint32_t perView)
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
    if (threadIdx.x < 32)
        s_exp[threadIdx.x] = kExp2fTab[threadIdx.x];
    __syncthreads();

    // this block's view: its radiance and its plane
    ps.rad += (size_t)blockIdx.y*perView;
    accum += (size_t)blockIdx.y*(size_t)(fp.width*fp.height);

    const AccTile g = tile_geometry(fp, nullptr);
    const int side = g.side, reachLo = g.reachLo;

    // the (at most two) candidate entries this thread stages every pass: entry t, t + 256
    AccEntries<kEnt> ent;
    bool entStage[kEnt];
#pragma unroll
    for (int k = 0; k < kEnt; ++k)
    {
        const int e = threadIdx.x + k*kBlock;
        const int ex = e % side, ey = e/side;
        ent.gx[k] = g.ox + ex; ent.gy[k] = g.oy + ey;
        ent.le[k] = ey*kSide + ex;
        ent.live[k] = e < side*side && candidate_live(fp, ent.gx[k], ent.gy[k]);
        entStage[k] = e < side*side;                    // (entries outside the frame are staged as "covers nothing", every pass)
    }
    ent.request(ps, fp, fp.accBegin);

    const int lx = threadIdx.x % kAccTile, ly = threadIdx.x/kAccTile;
    const int px = g.tx*kAccTile + lx, py = g.ty*kAccTile + ly;
    const bool inside = px < fp.width && py < fp.height;

    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (inside)
        acc = accum[py*fp.width + px];

    // this pixel's candidate window, in LDS coordinates (clipped to the frame like the reference's loops)
    const int i0 = maxI(0, px - reachLo) - g.ox, i1 = minI(fp.width - 1, px + g.reachHi) - g.ox;
    const int j0 = maxI(0, py - reachLo) - g.oy, j1 = minI(fp.height - 1, py + g.reachHi) - g.oy;

    for (int s = fp.accBegin; s < fp.accEnd; ++s)
    {
        float4 curRa[kEnt];
        ent.rotate(ps, fp, s, curRa);

#pragma unroll
        for (int k = 0; k < kEnt; ++k)
        {
            if (!entStage[k])
                continue;
            const int le = ent.le[k];
            float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);     // nX == 0: covers nothing
            uint32_t ym = 0;
            if (ent.live[k])
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

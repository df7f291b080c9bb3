// tn_features.h -- k_features: the first-hit features of the camera's own paths (tinsel_hip_render_features*).
//
// The guide buffers a denoiser or a compositor takes beside the beauty -- albedo, shading normal, depth, coverage -- have to be reconstructed
// exactly as the beauty is: the same camera sample per (pass, pixel), the same shutter time, the same filter weights.  So the kernel makes
// no image.  One lane per path slot (slot_pixel, as k_cost enumerates them; tile padding returns): camera_sample as begin_path runs it -- seed
// Random(i + j*W + pass_seed(s)), draws x, y, t --, one closest-hit trace<> at the sample's time (k_query's), and per requested plane one
// 16-byte record by slot:
//   kFeatureAlbedo   the bits of the hit primitive's material colour (Mat128::color = tinsel_material.color), 0
//   kFeatureNormal   FaceForward(n, -d): trace<>'s normal, what tinsel_ray_hit carries for that ray, 0
//   kFeatureDepth    t, t*t (one multiply), 1, 0 -- so that the plane's z/w is the coverage, x/z the mean depth over hits, y/z - (x/z)^2 its variance
// and (0, 0, 0, 0) in every plane at a miss.  The host then sends every plane through the accumulate kernels (tn_accumulate.h: the per-slot
// array is their `rad`), which add it with AddSample's arithmetic at the pass's raster position.
// The planes lie one after the other, `planeStride` records apart, each in slot order: a wave's store to a plane is one run of 64 records.
// Stores are typed as HBM (GlobalF4Out, tn_query.h); the mask is a kernel argument, so the branches around them are scalar.
// LDS as k_query: [stackEntries][kBlock] stack words, kScanWords, the staged arena.  Nothing but `out` is written: no statistics, no path state.
#pragma once

#include "tn_query.h"

namespace tn {

enum FeatureBit : uint32_t { kFeatureAlbedo = 1u, kFeatureNormal = 2u, kFeatureDepth = 4u, kFeatureAll = 7u };

struct FeatureJob
{
    void* out;                  // float4[popcount(mask)][planeStride]: the requested planes in ascending bit order
    uint32_t planeStride;       // records from one plane to the next (the batch buffer's slots)
    uint32_t mask;              // FeatureBit
};

template <bool LDS>
__global__ __launch_bounds__(kBlock, TN_WAVES_TRACE) void k_features(DevScene scIn, FeatureJob job, CameraParams cam, FrameParams fp,
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
    const bool hit = prim >= 0;

    GlobalF4Out op = (GlobalF4Out)(uintptr_t)job.out + idx;
    if (job.mask & kFeatureAlbedo)
    {
        WalkF4 r;
        r.x = 0.0f; r.y = 0.0f; r.z = 0.0f; r.w = 0.0f;
        if (hit)
        {
            const float4 c = reinterpret_cast<const float4*>(sc.mats + prim)[1];       // Mat128: color, metallic
            r.x = c.x; r.y = c.y; r.z = c.z;
        }
        *op = r;
        op += job.planeStride;
    }
    if (job.mask & kFeatureNormal)
    {
        WalkF4 r;
        r.x = hit ? n.x : 0.0f;
        r.y = hit ? n.y : 0.0f;
        r.z = hit ? n.z : 0.0f;
        r.w = 0.0f;
        *op = r;
        op += job.planeStride;
    }
    if (job.mask & kFeatureDepth)
    {
        WalkF4 r;
        r.x = hit ? t : 0.0f;
        r.y = hit ? t*t : 0.0f;
        r.z = hit ? 1.0f : 0.0f;
        r.w = 0.0f;
        *op = r;
    }
}

} // namespace tn

// tn_host_denoise.h -- the feature-guided denoise stage (tinsel_hip_denoise*, tn_denoise.h): arguments, buffers, launches
// (part of the library's one host translation unit: included by tinsel_hip.hip, in this order, never on its own)
#pragma once

namespace {

inline tinsel_hip_denoise_params denoise_defaults()
{
    // chosen on host renders of the reference (profiles/denoise_defaults.md)
    tinsel_hip_denoise_params p;
    p.radius = 8;
    p.patch_radius = 1;
    p.k_color = 2.0f;
    p.k_albedo = 4.0f;
    p.k_normal = 8.0f;
    p.k_depth = 1.0f;
    p.demodulate = 0;
    p.albedo_floor = 0.5f;
    return p;
}

// the refusals of both entries that need no renderer: -1 before anything is written or launched
int denoise_args(const tinsel_hip* r, const void* planes, unsigned features, int width, int height, const tinsel_hip_denoise_params* p, const void* out,
                 const char* who)
{
    const std::string w(who);
    if (!r || !p || !out)
        return fail(w + ": null argument");
    if (features > (unsigned)kFeatureAll)
        return fail(w + ": features must be a set of TINSEL_FEATURE_ALBEDO | _NORMAL | _DEPTH");
    if (!planes && features != 0u)
        return fail(w + ": null argument (planes may be NULL only with features == 0)");
    if (p->radius < 1 || p->radius > kDenoiseMaxRadius)
        return fail(w + ": params.radius must be 1 .. 8");
    if (p->patch_radius < 0 || p->patch_radius > kDenoiseMaxPatch)
        return fail(w + ": params.patch_radius must be 0 .. 4");
    for (const float k : { p->k_color, p->k_albedo, p->k_normal, p->k_depth })
        if (!std::isfinite(k) || k < 0.0f)
            return fail(w + ": params.k_color, k_albedo, k_normal and k_depth must be finite and >= 0");
    if (p->demodulate != 0 && p->demodulate != 1)
        return fail(w + ": params.demodulate must be 0 or 1");
    if (!std::isfinite(p->albedo_floor) || !(p->albedo_floor > 0.0f))
        return fail(w + ": params.albedo_floor must be finite and > 0");
    if (p->demodulate && !(features & TINSEL_FEATURE_ALBEDO))
        return fail(w + ": params.demodulate needs the albedo plane (TINSEL_FEATURE_ALBEDO in features)");
    if (width <= 0 || height <= 0 || (size_t)width*(size_t)height > (size_t)0x7fffffff)
        return fail(w + ": width and height must be positive (and width*height below 2^31)");
    return 0;
}

// ... and the one that looks at the renderer: beauty == NULL names the accumulator
int denoise_own_beauty(const tinsel_hip* r, int width, int height, const char* who)
{
    if (!r->accum || width != r->width || height != r->height)
        return fail(std::string(who) + ": beauty == NULL is the renderer's accumulator: width/height do not match the last tinsel_hip_init");
    return 0;
}

template <unsigned MASK>
void launch_denoise(dim3 grid, size_t lds, hipStream_t st, const float4* means, const float4* u, const float4* ga, const float4* gn, float4* out, int width,
                    int height, const DenoiseParams& dp)
{
    hipLaunchKernelGGL(k_denoise<MASK>, grid, dim3(256), lds, st, means, u, ga, gn, out, width, height, dp);
}

// Enqueues on st: prepare, the patch means, the filter.  The four intermediate images are the renderer's, kept until tinsel_hip_destroy; two
// calls on two streams share them: the later one's stream waits for the event behind the earlier one's last launch.  Every input is read
// by the first kernel, the output written by the last: `out` may be any of the inputs.
int denoise_enqueue(tinsel_hip* r, const float4* beauty, const float4* planes, unsigned features, int width, int height, const tinsel_hip_denoise_params* p,
                    float4* out, hipStream_t st)
{
    const size_t npix = (size_t)width*height;
    for (DevBuf<float4>& b : r->denoise)
    {
        // (a buffer that grows may still be read by an earlier call's launches)
        if (b && b.count() < npix)
            HIP_TRY(hipDeviceSynchronize());
        if (b.grow(npix))
            return -1;
    }
    if (r->denoiseFence.create())
        return -1;
    if (r->denoiseFencePending && r->denoiseFenceStream != st)
        HIP_TRY(hipStreamWaitEvent(st, r->denoiseFence, 0));

    const float4* plane[3] = { nullptr, nullptr, nullptr };
    for (int bit = 0, k = 0; bit < 3; ++bit)
        if (features >> bit & 1u)
            plane[bit] = planes + npix*(size_t)k++;
    float4* const u = r->denoise[0].get();
    float4* const means = r->denoise[1].get();
    float4* const ga = r->denoise[2].get();
    float4* const gn = r->denoise[3].get();

    DenoiseParams dp;
    dp.radius = p->radius; dp.patchRadius = p->patch_radius;
    dp.kColor = p->k_color; dp.kAlbedo = p->k_albedo; dp.kNormal = p->k_normal; dp.kDepth = p->k_depth;
    dp.demodulate = p->demodulate; dp.albedoFloor = p->albedo_floor;

    // (no class in tinsel_hip_kernel_times: the caller times the stage with events on its stream)
    hipLaunchKernelGGL(k_denoise_prepare, dim3((unsigned)((npix + 255)/256)), dim3(256), 0, st, beauty, plane[0], plane[1], plane[2], u, ga, gn, (int)npix,
                       dp.demodulate, dp.albedoFloor);
    hipLaunchKernelGGL(k_nlm_means, dim3((width + 15)/16, (height + 15)/16), dim3(256), 0, st, u, means, width, height, dp.patchRadius);
    const dim3 grid((width + kDenoiseTileW - 1)/kDenoiseTileW, (height + kDenoiseTileH - 1)/kDenoiseTileH);
    const size_t lds = denoise_lds_bytes(features, dp.radius);
    switch (features)
    {
    case 0: launch_denoise<0>(grid, lds, st, means, u, ga, gn, out, width, height, dp); break;
    case 1: launch_denoise<1>(grid, lds, st, means, u, ga, gn, out, width, height, dp); break;
    case 2: launch_denoise<2>(grid, lds, st, means, u, ga, gn, out, width, height, dp); break;
    case 3: launch_denoise<3>(grid, lds, st, means, u, ga, gn, out, width, height, dp); break;
    case 4: launch_denoise<4>(grid, lds, st, means, u, ga, gn, out, width, height, dp); break;
    case 5: launch_denoise<5>(grid, lds, st, means, u, ga, gn, out, width, height, dp); break;
    case 6: launch_denoise<6>(grid, lds, st, means, u, ga, gn, out, width, height, dp); break;
    default: launch_denoise<7>(grid, lds, st, means, u, ga, gn, out, width, height, dp); break;
    }
    // (whatever was enqueued reads and writes the stage's buffers: the next call waits for it)
    if (hipEventRecord(r->denoiseFence, st) == hipSuccess)
    {
        r->denoiseFenceStream = st;
        r->denoiseFencePending = true;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

} // namespace

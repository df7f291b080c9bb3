// tn_host_features.h -- feature buffers (tinsel_hip_render_features*): albedo, normal and depth on the beauty's own samples
// (part of the library's one host translation unit: included by tinsel_hip.hip, in this order, never on its own)
#pragma once

namespace {

// Enqueues on st: the planes `features` asks for of the passes [passBegin, passBegin + passes) into target[plane][H][W] (device, 16-byte
// aligned), each plane from zero.  Per batch of whole passes (passes_per_batch, side_pass_batches) k_features writes one
// 16-byte record per requested plane and path slot into r->featRec (tn_features.h), and one launch_accumulate per plane adds that plane's
// records to its part of `target` exactly as a render adds a batch's radiance to the accumulator: the call's own seeds for the raster
// positions, options->filter for the weights, and a clamp of +infinity, which ClampLength's `l > max` never meets.  Batches follow each
// other on st and every pixel's adds stay in pass order, so the cut shows nowhere.
// The seeds are the call's own table, pass_seed(passBegin + s), made on the device by k_pass_seeds from seed_rng_at's copy of the
// renderer's generator; the records and the table are the call's own buffers, kept until tinsel_hip_destroy, so neither the path
// buffers nor the renderer's seed table are touched and nothing of a render or a look-ahead in flight has to be waited for.  Two calls on
// two streams share those buffers: the later one's stream waits for the event behind the earlier one's last launch.
int features_enqueue(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options, uint32_t passBegin, int passes, unsigned features,
                     float4* target, hipStream_t st)
{
    const size_t npix = (size_t)r->width*r->height;
    const int planes = __builtin_popcount(features);

    CameraParams cam;
    make_camera(*camera, options->width, options->height, cam);
    FrameParams fp = frame_params(r, options);
    fp.clampLen = INFINITY;

    const size_t perPass = slots_per_pass(r, fp.width, fp.height);
    const int perBatch = passes_per_batch(batch_slots(r), perPass, passes);
    const size_t stride = perPass*(size_t)perBatch;
    if (stride >= (size_t)0xffffffffu)
        return fail("render_features: batch too large");

    // (grown before the first wait on a stream; a buffer that grows may still be read by an earlier call's launches)
    if (query_buffer(r->featRec, stride*(size_t)planes*sizeof(float4)))
        return -1;
    if (r->featSeeds.count() < (size_t)passes)
    {
        if (r->featSeeds)
            HIP_TRY(hipDeviceSynchronize());
        if (r->featSeeds.alloc((size_t)passes))
            return -1;
    }
    if (r->featFence.create())
        return -1;
    if (r->featFencePending && r->featFenceStream != st)
        HIP_TRY(hipStreamWaitEvent(st, r->featFence, 0));

    const Rng g = seed_rng_at(r, passBegin);
    hipLaunchKernelGGL(k_pass_seeds, dim3(1), dim3(1), 0, st, g.s1, g.s2, passes, r->featSeeds.get());
    HIP_TRY(hipMemsetAsync(target, 0, sizeof(float4)*npix*(size_t)planes, st));

    float4* const rec = (float4*)r->featRec.get();
    const int rc = side_pass_batches(r, cam, fp, passes, perBatch, r->featSeeds.get(), PK_FEATURES_LDS, PK_FEATURES, "render_features",
                                     [&](LaunchArgs& a, const FrameParams& batch) {
        a.features.out = rec;
        a.features.planeStride = (uint32_t)stride;
        a.features.mask = features;
        {
            ScopedTimer t(r, KN_FEATURES, st);
            if (launch_path(r, a, st))
                return -1;
        }
        for (int p = 0; p < planes; ++p)
            if (launch_accumulate(r, st, batch, rec + (size_t)p*stride, target + (size_t)p*npix, r->featSeeds.get()))
                return -1;
        return 0;
    });
    // (whatever was enqueued reads the call's buffers: the next call waits for it, failed or not)
    if (hipEventRecord(r->featFence, st) == hipSuccess)
    {
        r->featFenceStream = st;
        r->featFencePending = true;
    }
    if (rc)
        return -1;
    HIP_TRY(hipGetLastError());
    return 0;
}

// the refusals of both entries: -1 before anything is written or launched
int features_args(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options, int passes, unsigned features, const void* out, const char* who)
{
    const std::string w(who);
    if (!r || !camera || !options || !out)
        return fail(w + ": null argument");
    if (passes < 1)
        return fail(w + ": passes must be >= 1");
    if (features == 0u || features > (unsigned)kFeatureAll)
        return fail(w + ": features must be a non-empty set of TINSEL_FEATURE_ALBEDO | _NORMAL | _DEPTH");
    if (options->mode != TINSEL_MODE_PATHTRACE)
        return fail(w + ": options.mode must be TINSEL_MODE_PATHTRACE");
    if (!r->accum || options->width != r->width || options->height != r->height)
        return fail(w + ": options.width/height do not match the last tinsel_hip_init");
    return 0;
}

} // namespace

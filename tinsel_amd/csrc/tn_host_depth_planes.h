// tn_host_depth_planes.h -- depth planes (tinsel_hip_render_depth_planes*): the beauty at several path depths in one trace
// (part of the library's one host translation unit: included by tinsel_hip.hip, in this order, never on its own)
#pragma once

namespace {

// bit d - 1 for every depth asked for (DepthState::mask); the caller has checked the list (depth_planes_args)
uint64_t depth_mask(int numPlanes, const int32_t* depths)
{
    uint64_t m = 0;
    for (int k = 0; k < numPlanes; ++k)
        m |= 1ull << (depths[k] - 1);
    return m;
}

// Enqueues on st: plane k of target[plane][H][W] (device, 16-byte aligned) = the accumulator of the passes [passBegin, passBegin + passes)
// rendered with max_depth = depths[k], from zero or (TINSEL_DEPTH_PLANES_ADD) on top of what the plane holds.  Per batch of whole passes the
// camera's paths are traced ONCE, to depths[last], through the split pipeline with k_shade_depths as its shading kernel (plan_batch's
// SIDE_DEPTHS, trace_batch's TraceOverrides): it leaves in r->depthsRec[k*stride + slot] the path's radiance after the bounce depths[k] - 1,
// every record written exactly once, so nothing is zeroed.  Then one k_views_accumulate launch with the planes as its second grid
// dimension -- or, for filters whose halo does not fit and under TINSEL_DEPTH_PLANES_ACCUMULATE_SINGLY, one launch_accumulate per plane --
// adds each plane's records to its part of `target` exactly as a render adds a batch's radiance to the accumulator: the call's own seeds
// for the raster positions, options' filter AND clamp.  Batches follow each other on st and every pixel's adds stay in pass order, so the
// cut shows nowhere.
// Seeds, records and fence as light_groups_enqueue (tn_host_light_groups.h); the paths live in the renderer's path buffers, which the call
// takes and leaves as a radiance query does (ensure_batch, batch_fence_wait / own_streams_wait, batch_fence_signal).  The statistics of its
// kernels go to a block of the call's own that nobody reads.
int depth_planes_enqueue(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options, uint32_t passBegin, int passes, int numPlanes,
                         const int32_t* depths, int flags, float4* target, hipStream_t st)
{
    const size_t npix = (size_t)r->width*r->height;
    const bool add = (flags & TINSEL_DEPTH_PLANES_ADD) != 0;

    CameraParams cam;
    make_camera(*camera, options->width, options->height, cam);
    FrameParams fp = frame_params(r, options);
    fp.maxDepth = depths[numPlanes - 1];            // (options->max_depth is not read)
    const bool singly = (flags & TINSEL_DEPTH_PLANES_ACCUMULATE_SINGLY) != 0 || !accumulate_tiled_fits(fp);

    const size_t perPass = slots_per_pass(r, fp.width, fp.height);
    const size_t slotLimit = batch_slots(r)*kPathStateBytes/(kPathStateBytes + sizeof(float4)*(size_t)numPlanes);
    const int perBatch = passes_per_batch(slotLimit, perPass, passes);
    const size_t stride = perPass*(size_t)perBatch;
    if (stride >= (size_t)0xffffffffu)
        return fail("render_depth_planes: batch too large");

    // (grown before the first wait on a stream; a buffer that grows may still be read by an earlier call's launches)
    if (query_buffer(r->depthsRec, stride*(size_t)numPlanes*sizeof(float4)))
        return -1;
    if (r->depthsSeeds.count() < (size_t)passes)
    {
        if (r->depthsSeeds)
            HIP_TRY(hipDeviceSynchronize());
        if (r->depthsSeeds.alloc((size_t)passes))
            return -1;
    }
    if (!r->depthsStats && r->depthsStats.alloc((size_t)kStatShards*kStatWords))
        return -1;
    if (r->depthsFence.create())
        return -1;

    const BatchPlan plan = plan_batch(r, perPass, perBatch, /*mayOverlap*/ false, PK_GENERATE, SIDE_DEPTHS);
    if (ensure_batch(r, plan, fp.maxDepth) || batch_fence_wait(r, st) || own_streams_wait(r, st))
        return -1;
    if (r->depthsFencePending && r->depthsFenceStream != st)
        HIP_TRY(hipStreamWaitEvent(st, r->depthsFence, 0));

    const Rng g = seed_rng_at(r, passBegin);
    hipLaunchKernelGGL(k_pass_seeds, dim3(1), dim3(1), 0, st, g.s1, g.s2, passes, r->depthsSeeds.get());
    if (!add)
        HIP_TRY(hipMemsetAsync(target, 0, sizeof(float4)*npix*(size_t)numPlanes, st));

    float4* const rec = (float4*)r->depthsRec.get();
    TraceOverrides over;
    over.passSeeds = r->depthsSeeds.get();
    over.stats = r->depthsStats.get();
    over.depths = { rec, depth_mask(numPlanes, depths), (uint32_t)stride };

    // (what the renderer remembers of its last batch -- look-ahead's accumulate, the test hooks -- is a render's, not this call's)
    const FrameParams keptFp = r->lastFp;
    const int keptPipeline = r->lastPipeline, keptLane = r->lastLane;
    int rc = 0;
    for (int done = 0; done < passes && !rc; done += perBatch)
    {
        FrameParams batch = fp;
        batch.passBase = done;
        batch.numPasses = std::min(perBatch, passes - done);
        const size_t slots = batch_frame(r, batch);
        if (!slots)
        {
            rc = fail("render_depth_planes: batch too large");
            break;
        }
        // (a finished path's radiance is in the planes: k_shade_depths does not write radOut; ps.rad is there for k_generate's signature)
        rc = trace_batch(r, plan, r->lane[0], st, &cam, batch, r->ps.rad, slots, nullptr, &over);
        if (!rc && !singly)
            rc = launch_views_accumulate(r, st, batch, rec, target, r->depthsSeeds.get(), numPlanes, stride);
        for (int p = 0; p < numPlanes && !rc && singly; ++p)
            rc = launch_accumulate(r, st, batch, rec + (size_t)p*stride, target + (size_t)p*npix, r->depthsSeeds.get());
    }
    r->lastFp = keptFp;
    r->lastPipeline = keptPipeline;
    r->lastLane = keptLane;

    // (whatever was enqueued reads the call's buffers and the path buffers: the next user waits for it, failed or not)
    if (hipEventRecord(r->depthsFence, st) == hipSuccess)
    {
        r->depthsFenceStream = st;
        r->depthsFencePending = true;
    }
    if (batch_fence_signal(r, st) || rc)
        return -1;
    HIP_TRY(hipGetLastError());
    return 0;
}

// the refusals of both entries: -1 before anything is written or launched
int depth_planes_args(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options, int passes, int numPlanes, const int32_t* depths,
                      int flags, const void* out, const char* who)
{
    const std::string w(who);
    if (!r || !camera || !options || !depths || !out)
        return fail(w + ": null argument");
    if (passes < 1)
        return fail(w + ": passes must be >= 1");
    if (numPlanes < 1 || numPlanes > TINSEL_MAX_DEPTH_PLANES)
        return fail(w + ": num_planes must be in 1 .. TINSEL_MAX_DEPTH_PLANES");
    for (int k = 0; k < numPlanes; ++k)
        if (depths[k] < 1 || depths[k] > TINSEL_MAX_PLANE_DEPTH || (k > 0 && depths[k] <= depths[k - 1]))
            return fail(w + ": depths[" + std::to_string(k) + "] must be in 1 .. TINSEL_MAX_PLANE_DEPTH and above the entry before it");
    if (flags & ~(TINSEL_DEPTH_PLANES_ADD | TINSEL_DEPTH_PLANES_ACCUMULATE_SINGLY))
        return fail(w + ": unknown flag bits");
    if (options->mode != TINSEL_MODE_PATHTRACE)
        return fail(w + ": options.mode must be TINSEL_MODE_PATHTRACE");
    if (!r->accum || options->width != r->width || options->height != r->height)
        return fail(w + ": options.width/height do not match the last tinsel_hip_init");
    if (r->shardWorld > 1)
        return fail(w + ": a sharded renderer (world > 1) has no depth planes");
    if (r->arith != TINSEL_ARITH_EXACT)
        return fail(w + ": the tolerance arithmetic arm (TINSEL_ARITH_FAST) has no depth planes");
    return 0;
}

} // namespace

// tn_host_light_groups.h -- light groups (tinsel_hip_render_light_groups*): the beauty split per emitter group in one trace
// (part of the library's one host translation unit: included by tinsel_hip.hip, in this order, never on its own)
#pragma once

namespace {

// what a path slot's own dense state weighs beside the planes' 16 bytes per group: five 16-byte records in two buffers and the radiance
constexpr size_t kPathStateBytes = 176;

// Enqueues on st: the planes of the passes [passBegin, passBegin + passes) into target[group][H][W] (device, 16-byte aligned), each plane
// from zero.  Per batch of whole passes the planes' records (r->groupsRec: [g*stride + slot], as the accumulate kernels read a batch's
// radiance) are zeroed, the camera's paths are traced through the split pipeline with k_shade_groups as its shading kernel (plan_batch's
// `groups`, trace_batch's TraceOverrides), and one launch_accumulate per plane adds that plane's records to its part of `target` exactly as
// a render adds a batch's radiance to the accumulator: the call's own seeds for the raster positions, options' filter AND clamp.  Batches
// follow each other on st and every pixel's adds stay in pass order, so the cut shows nowhere.
// Seeds, records, table and fence as features_enqueue (tn_host_features.h); the paths live in the renderer's path buffers, which the call
// takes and leaves as a radiance query does (ensure_batch, batch_fence_wait / own_streams_wait, batch_fence_signal).  The statistics of its
// kernels go to a block of the call's own that nobody reads.
int light_groups_enqueue(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options, uint32_t passBegin, int passes, int numGroups,
                         const int32_t* groupOf, int envGroup, float4* target, hipStream_t st)
{
    const size_t npix = (size_t)r->width*r->height;

    CameraParams cam;
    make_camera(*camera, options->width, options->height, cam);
    FrameParams fp = frame_params(r, options);

    if (fp.maxDepth < 1)
    {
        HIP_TRY(hipMemsetAsync(target, 0, sizeof(float4)*npix*(size_t)numGroups, st));      // no bounce, no term
        return 0;
    }

    const size_t perPass = slots_per_pass(r, fp.width, fp.height);
    const size_t slotLimit = batch_slots(r)*kPathStateBytes/(kPathStateBytes + sizeof(float4)*(size_t)numGroups);
    const int perBatch = passes_per_batch(slotLimit, perPass, passes);
    const size_t stride = perPass*(size_t)perBatch;
    if (stride >= (size_t)0xffffffffu)
        return fail("render_light_groups: batch too large");

    // (grown before the first wait on a stream; a buffer that grows may still be read by an earlier call's launches)
    if (query_buffer(r->groupsRec, stride*(size_t)numGroups*sizeof(float4)))
        return -1;
    if (r->groupsSeeds.count() < (size_t)passes)
    {
        if (r->groupsSeeds)
            HIP_TRY(hipDeviceSynchronize());
        if (r->groupsSeeds.alloc((size_t)passes))
            return -1;
    }
    if (!r->groupsStats && r->groupsStats.alloc((size_t)kStatShards*kStatWords))
        return -1;
    if (r->groupsFence.create())
        return -1;

    // the primitives' groups, one byte each; uploaded where they differ from what the device holds, after whatever still reads that
    std::vector<int8_t> table(r->primsHost.size());
    for (size_t i = 0; i < table.size(); ++i)
        table[i] = (int8_t)groupOf[i];
    if (!r->groupsTable || table != r->groupsTableHost)
    {
        if (r->groupsFencePending)
            HIP_TRY(hipEventSynchronize(r->groupsFence));
        r->groupsTableHost.clear();
        if (r->groupsTable.upload(table.data(), table.size()))
            return -1;
        r->groupsTableHost = table;
    }

    const BatchPlan plan = plan_batch(r, perPass, perBatch, /*mayOverlap*/ false, PK_GENERATE, SIDE_GROUPS);
    if (ensure_batch(r, plan, fp.maxDepth) || batch_fence_wait(r, st) || own_streams_wait(r, st))
        return -1;
    if (r->groupsFencePending && r->groupsFenceStream != st)
        HIP_TRY(hipStreamWaitEvent(st, r->groupsFence, 0));

    const Rng g = seed_rng_at(r, passBegin);
    hipLaunchKernelGGL(k_pass_seeds, dim3(1), dim3(1), 0, st, g.s1, g.s2, passes, r->groupsSeeds.get());
    HIP_TRY(hipMemsetAsync(target, 0, sizeof(float4)*npix*(size_t)numGroups, st));

    float4* const rec = (float4*)r->groupsRec.get();
    TraceOverrides over;
    over.passSeeds = r->groupsSeeds.get();
    over.stats = r->groupsStats.get();
    over.groups = { rec, r->groupsTable.get(), envGroup, (uint32_t)stride };

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
            rc = fail("render_light_groups: batch too large");
            break;
        }
        if (hipMemsetAsync(rec, 0, stride*(size_t)numGroups*sizeof(float4), st) != hipSuccess)
        {
            rc = fail("render_light_groups: hipMemsetAsync");
            break;
        }
        // (a finished path's own radiance goes nowhere: k_shade_groups does not write radOut; ps.rad is there for k_generate's signature)
        rc = trace_batch(r, plan, r->lane[0], st, &cam, batch, r->ps.rad, slots, nullptr, &over);
        for (int p = 0; p < numGroups && !rc; ++p)
            rc = launch_accumulate(r, st, batch, rec + (size_t)p*stride, target + (size_t)p*npix, r->groupsSeeds.get());
    }
    r->lastFp = keptFp;
    r->lastPipeline = keptPipeline;
    r->lastLane = keptLane;

    // (whatever was enqueued reads the call's buffers and the path buffers: the next user waits for it, failed or not)
    if (hipEventRecord(r->groupsFence, st) == hipSuccess)
    {
        r->groupsFenceStream = st;
        r->groupsFencePending = true;
    }
    if (batch_fence_signal(r, st) || rc)
        return -1;
    HIP_TRY(hipGetLastError());
    return 0;
}

// the refusals of both entries: -1 before anything is written or launched
int light_groups_args(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options, int passes, int numGroups, const int32_t* groupOf,
                      int envGroup, const void* out, const char* who)
{
    const std::string w(who);
    if (!r || !camera || !options || !groupOf || !out)
        return fail(w + ": null argument");
    if (passes < 1)
        return fail(w + ": passes must be >= 1");
    if (numGroups < 1 || numGroups > TINSEL_MAX_LIGHT_GROUPS)
        return fail(w + ": num_groups must be in 1 .. TINSEL_MAX_LIGHT_GROUPS");
    if (envGroup < -1 || envGroup >= numGroups)
        return fail(w + ": env_group must be in -1 .. num_groups - 1");
    if (options->mode != TINSEL_MODE_PATHTRACE)
        return fail(w + ": options.mode must be TINSEL_MODE_PATHTRACE");
    if (!r->accum || options->width != r->width || options->height != r->height)
        return fail(w + ": options.width/height do not match the last tinsel_hip_init");
    for (size_t i = 0; i < r->primsHost.size(); ++i)
        if (groupOf[i] < -1 || groupOf[i] >= numGroups)
            return fail(w + ": group_of_primitive[" + std::to_string(i) + "] must be in -1 .. num_groups - 1");
    if (r->shardWorld > 1)
        return fail(w + ": a sharded renderer (world > 1) has no light groups");
    if (r->arith != TINSEL_ARITH_EXACT)
        return fail(w + ": the tolerance arithmetic arm (TINSEL_ARITH_FAST) has no light groups");
    return 0;
}

} // namespace

// tn_host_radiance.h -- radiance queries (tinsel_hip_trace_radiance*): PathTrace() for paths the caller starts, on the scene in force
// (part of the library's one host translation unit: included by tinsel_hip.hip, in this order, never on its own)
#pragma once

namespace {

// paths per chunk of the host entry: 48 MB of starts + 16 MB of radiance on the device, whatever n is
constexpr size_t kRadianceChunk = (size_t)1 << 20;

static_assert(sizeof(tinsel_path_start) == 3*sizeof(float4), "k_generate_rays reads a record as three 16-byte loads");

// A query runs the paired pipeline where a render would, and the split pipeline in every other case -- also on a scene a render takes
// through the fused kernel, and under a MEGAKERNEL setting: k_bounce and k_mega make the camera's paths inside the kernel, the split and
// the paired pipeline in ONE kernel in front of everything else (k_generate), which k_generate_rays stands in for.
int radiance_pipeline(const tinsel_hip* r)
{
    return resolve_pipeline(r) == TINSEL_PIPELINE_WAVEFRONT_PAIRED ? TINSEL_PIPELINE_WAVEFRONT_PAIRED : TINSEL_PIPELINE_WAVEFRONT_SPLIT;
}

// Enqueues the paths starts[0, n) on st: out[k] = PathTrace(starts[k]), both device arrays.  The paths are traced in the renderer's path
// buffers, batch_slots() at a time, one batch after the other on st -- a path's result is a function of its record alone, so the cut shows
// nowhere.  Ordered against the buffers' other users by events, both ways and without a host wait: st waits for what the renderer has in
// flight (the default stream's, the look-ahead's, a render or a query on a caller's stream: batch_fence_wait), nothing of it is
// discarded, and the fence recorded behind the last launch is what the next user waits for.
int trace_radiance(tinsel_hip* r, size_t n, const void* starts, float4* out, int maxDepth, hipStream_t st)
{
    const size_t perBatch = std::min(n, batch_slots(r));
    BatchPlan plan = plan_batch(r, perBatch, 1, /*mayOverlap*/ false, radiance_pipeline(r));
    plan.generate = PK_GENERATE_RAYS;
    if (ensure_batch(r, plan, maxDepth) || batch_fence_wait(r, st))
        return -1;
    const hipStream_t own[2] = { nullptr, (hipStream_t)r->workStream };
    for (int k = 0; k < 2; ++k)
    {
        if (own[k] == st || (k == 1 && !own[k]))
            continue;
        if (r->queryFork[k].create())
            return -1;
        HIP_TRY(hipEventRecord(r->queryFork[k], own[k]));
        HIP_TRY(hipStreamWaitEvent(st, r->queryFork[k], 0));
    }

    // no pixel, no pass, no shard: the generation count, the depth and the roulette start are all the kernels behind k_generate_rays read
    FrameParams fp;
    memset(&fp, 0, sizeof(fp));
    fp.maxDepth = maxDepth;
    fp.rrStart = r->rrStart;
    fp.numPasses = 1;
    fp.shardWorld = 1;
    for (size_t done = 0; done < n; done += perBatch)
    {
        const size_t m = std::min(perBatch, n - done);
        const RadianceJob job = { starts, (uint32_t)done, (uint32_t)m };
        CallerPaths paths;
        paths.rays = &job;
        fp.genCount = (uint32_t)m;
        r->lastLane = 0;
        // (ss.radOut is the caller's array at the batch's first record: a finished path writes out[done + slot] itself)
        if (trace_batch(r, plan, r->lane[0], st, nullptr, fp, out + done, m, &paths))
            return -1;
    }
    HIP_TRY(hipGetLastError());
    return batch_fence_signal(r, st);
}

int radiance_args(tinsel_hip* r, long long n, const void* starts, const void* out, int maxDepth, const char* who)
{
    if (!r || n < 0 || n > 0x7fffffffll || maxDepth < 1 || (n > 0 && (!starts || !out)))
        return fail(std::string(who) + ": bad arguments (a renderer, 0 <= n < 2^31, max_depth >= 1, two arrays)");
    return 0;
}

} // namespace

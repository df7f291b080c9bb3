// tn_host_gather.h -- gather queries (tinsel_hip_gather_radiance*): S paths from each of n surface points, drawn and reduced on the device
// (part of the library's one host translation unit: included by tinsel_hip.hip, in this order, never on its own)
#pragma once

namespace {

// The host entry's staging, at most 64 MB on the device whatever n and S are: 2^20 points per chunk are 32 MB of points + 16 MB of means;
// with starts_out a point costs 32 + 16 + 48*S bytes, and the chunk is the largest number of points that keeps the sum below the ceiling
// (at S = 65536 one point's records are 3 MB: a chunk always holds at least 21)
constexpr size_t kGatherChunk = (size_t)1 << 20;
constexpr size_t kGatherCeiling = (size_t)64 << 20;
constexpr int kGatherMaxSamples = 65536;

static_assert(sizeof(tinsel_gather_point) == 2*sizeof(float4), "k_generate_gather reads a point as two 16-byte loads");

size_t gather_chunk(size_t n, int samples, bool startsOut)
{
    size_t chunk = std::min(n, kGatherChunk);
    if (startsOut)
        chunk = std::min(chunk, kGatherCeiling/(sizeof(tinsel_gather_point) + sizeof(float4) + sizeof(tinsel_path_start)*(size_t)samples));
    return chunk;
}

// Enqueues on st: out[k] = the mean of PathTrace over the `samples` paths of points[k], all device arrays; startsOut (or null) receives the
// generated record of path (k, s) at k*samples + s.  A batch holds whole points only, floor(batch_slots / samples) of them (one at least), and the
// batches run one after the other on st in the renderer's path buffers; finished paths write to r->gatherRad (not to the batch's own
// radiance array: a look-ahead chunk's radiance may be waiting there to be accumulated), which k_gather_reduce reads behind the
// pipeline.  A point's mean is a function of its record and `samples` alone, so the cut shows nowhere.  Ordered against the buffers'
// other users as trace_radiance is.
int trace_gather(tinsel_hip* r, int mode, size_t n, const void* points, int samples, int maxDepth, float4* out, void* startsOut, hipStream_t st)
{
    const size_t S = (size_t)samples;
    // (tinsel_hip_set_batch_paths takes as little as 1024: a batch is one whole point then, `samples` paths)
    const size_t perBatch = std::min(n, std::max<size_t>(1, batch_slots(r)/S));
    if (perBatch*S >= (size_t)0xffffffffu)
        return fail("gather_radiance: batch too large");
    BatchPlan plan = plan_batch(r, perBatch*S, 1, /*mayOverlap*/ false, radiance_pipeline(r));
    plan.generate = PK_GENERATE_GATHER;
    if (ensure_batch(r, plan, maxDepth) || query_buffer(r->gatherRad, perBatch*S*sizeof(float4)) || batch_fence_wait(r, st))
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

    // (as a radiance query: the generation count, the depth and the roulette start are all the kernels behind the generation kernel read)
    FrameParams fp;
    memset(&fp, 0, sizeof(fp));
    fp.maxDepth = maxDepth;
    fp.rrStart = r->rrStart;
    fp.numPasses = 1;
    fp.shardWorld = 1;
    float4* const rad = (float4*)r->gatherRad.get();
    for (size_t done = 0; done < n; done += perBatch)
    {
        const size_t m = std::min(perBatch, n - done);
        const GatherJob job = { points, startsOut, out, (uint32_t)done, (uint32_t)m, (uint32_t)samples, (uint32_t)mode };
        CallerPaths paths;
        paths.gather = &job;
        fp.genCount = (uint32_t)(m*S);
        r->lastLane = 0;
        if (trace_batch(r, plan, r->lane[0], st, nullptr, fp, rad, m*S, &paths))
            return -1;
        LaunchArgs a;
        memset(&a, 0, sizeof(a));
        a.ps.rad = rad;
        a.gather = job;
        a.grid = (int)((m + kBlock - 1)/kBlock);
        a.variant = PK_GATHER_REDUCE;
        ScopedTimer t(r, KN_GATHER_REDUCE, st);
        if (launch_path(r, a, st))
            return -1;
    }
    HIP_TRY(hipGetLastError());
    return batch_fence_signal(r, st);
}

int gather_args(tinsel_hip* r, int mode, long long n, const void* points, int samples, int maxDepth, const void* out, const char* who)
{
    if (!r || (mode != TINSEL_GATHER_COSINE && mode != TINSEL_GATHER_SPHERE) || n < 0 || n > 0x7fffffffll || samples < 1 || samples > kGatherMaxSamples ||
        maxDepth < 1 || (n > 0 && (!points || !out)))
        return fail(std::string(who) + ": bad arguments (a renderer, a mode, 0 <= n < 2^31, 1 <= samples <= 65536, max_depth >= 1, two arrays)");
    return 0;
}

} // namespace

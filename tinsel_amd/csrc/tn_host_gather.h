// tn_host_gather.h -- gather queries (tinsel_hip_gather_radiance*, tinsel_hip_gather_sh*): S paths from each of n surface points, drawn and reduced on the device
// (part of the library's one host translation unit: included by tinsel_hip.hip, in this order, never on its own)
#pragma once

namespace {

// The host entry's staging, at most 64 MB on the device whatever n and S are: a point costs 32 bytes + 16 per float4 it gets back (one mean,
// or the (order + 1)^2 coefficients of tinsel_hip_gather_sh) + with starts_out 48*S, and a chunk is the largest number of points, 2^20 at
// most, that keeps the sum below the ceiling: 2^20 for a plain gather (32 MB of points + 16 MB of means), 381300 for order 2
// (at S = 65536 one point's records are 3 MB: a chunk always holds at least 21)
constexpr size_t kGatherChunk = (size_t)1 << 20;
constexpr size_t kGatherCeiling = (size_t)64 << 20;
constexpr int kGatherMaxSamples = 65536;

static_assert(sizeof(tinsel_gather_point) == 2*sizeof(float4), "k_generate_gather reads a point as two 16-byte loads");

size_t gather_chunk(size_t n, int samples, bool startsOut, size_t outEach = 1)
{
    const size_t point = sizeof(tinsel_gather_point) + sizeof(float4)*outEach + (startsOut ? sizeof(tinsel_path_start)*(size_t)samples : 0);
    return std::min(n, std::min(kGatherChunk, kGatherCeiling/point));
}

// A gather's reduction: the mean (k_gather_reduce, one float4 per point) or its projection on the bands 0 .. order (k_gather_sh_reduce)
constexpr int kGatherMean = -1;
constexpr size_t gather_out_each(int order) { return order < 0 ? 1 : (size_t)((order + 1)*(order + 1)); }

// Enqueues on st: out[k] = the mean of PathTrace over the `samples` paths of points[k] (order kGatherMean), or out[k*C .. k*C + C) = the mean
// of PathTrace times the basis function at the path's direction (order 0 .. 2, C = (order + 1)^2), all device arrays; startsOut (or null) receives the
// generated record of path (k, s) at k*samples + s.  A batch holds whole points only, floor(batch_slots / samples) of them (one at least), and the
// batches run as a radiance query's do (trace_caller_batches, tn_host_batch.h); finished paths write to r->gatherRad (not to the batch's own
// radiance array: a look-ahead chunk's radiance may be waiting there to be accumulated), which the reduction reads behind the
// pipeline: k_gather_reduce one lane per point, k_gather_sh_reduce one wave per point.  A point's result is a function of its record and
// `samples` alone, so the cut shows nowhere.
int trace_gather(tinsel_hip* r, int mode, int order, size_t n, const void* points, int samples, int maxDepth, float4* out, void* startsOut, hipStream_t st)
{
    const bool sh = order != kGatherMean;
    const size_t S = (size_t)samples;
    // (tinsel_hip_set_batch_paths takes as little as 1024: a batch is one whole point then, `samples` paths)
    const size_t perBatch = std::min(n, std::max<size_t>(1, batch_slots(r)/S));
    if (perBatch*S >= (size_t)0xffffffffu)
        return fail(sh ? "gather_sh: batch too large" : "gather_radiance: batch too large");
    // (grown in front of the batch buffers, not behind them: both are host-side allocations made before the first wait on a stream)
    if (query_buffer(r->gatherRad, perBatch*S*sizeof(float4)))
        return -1;
    float4* const rad = (float4*)r->gatherRad.get();
    return trace_caller_batches(r, n, perBatch, S, PK_GENERATE_GATHER, maxDepth, st,
                                [&](const BatchPlan& plan, const FrameParams& fp, size_t done, size_t m) {
        const GatherJob job = { points, startsOut, out, (uint32_t)done, (uint32_t)m, (uint32_t)samples, (uint32_t)mode };
        CallerPaths paths;
        paths.gather = &job;
        if (trace_batch(r, plan, r->lane[0], st, nullptr, fp, rad, m*S, &paths))
            return -1;
        LaunchArgs a;
        memset(&a, 0, sizeof(a));
        a.ps.rad = rad;
        a.gather = job;
        a.shOrder = order;
        a.grid = (int)(sh ? m : (m + kBlock - 1)/kBlock);
        a.variant = sh ? PK_GATHER_SH_REDUCE : PK_GATHER_REDUCE;
        ScopedTimer t(r, sh ? KN_GATHER_SH_REDUCE : KN_GATHER_REDUCE, st);
        return launch_path(r, a, st);
    });
}

int gather_args(tinsel_hip* r, int mode, long long n, const void* points, int samples, int maxDepth, const void* out, const char* who)
{
    if (!r || (mode != TINSEL_GATHER_COSINE && mode != TINSEL_GATHER_SPHERE) || n < 0 || n > 0x7fffffffll || samples < 1 || samples > kGatherMaxSamples ||
        maxDepth < 1 || (n > 0 && (!points || !out)))
        return fail(std::string(who) + ": bad arguments (a renderer, a mode, 0 <= n < 2^31, 1 <= samples <= 65536, max_depth >= 1, two arrays)");
    return 0;
}

// (judged first by the SH entries: an order out of range never reaches trace_gather, where -1 names the plain mean)
int gather_sh_order(int order, const char* who)
{
    if (order < 0 || order > TINSEL_GATHER_SH_MAX_ORDER)
        return fail(std::string(who) + ": bad arguments (order is 0, 1 or 2)");
    return 0;
}

} // namespace

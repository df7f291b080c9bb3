// tn_host_samples.h -- sample maps (tinsel_hip_render_sample_map*): a per-pixel pass count on the resident scene in one call
// (part of the library's one host translation unit: included by tinsel_hip.hip, in this order, never on its own)
#pragma once

namespace {

// The batch cut of a sample-map call (tinsel_hip_plan_sample_map states it): runs of `levels` consecutive levels
struct SamplesCut
{
    unsigned long long levels = 1, batches = 0, paths = 0;
    uint32_t most = 0;          // the largest count of the map
};

// false: a level of the frame does not fit the 32-bit slot index.  The bound on a batch, levels*W*H, needs no histogram.
bool plan_samples(unsigned long long slotLimit, int width, int height, const uint16_t* counts, SamplesCut& c)
{
    const unsigned long long npix = (unsigned long long)width*(unsigned long long)height, top = 0xfffffffeull;     // (no batch has 2^32 - 1 slots or more)
    if (npix > top)
        return false;
    c.levels = std::max(1ull, std::min(slotLimit, top)/npix);
    c.paths = 0;
    c.most = 0;
    for (unsigned long long q = 0; q < npix; ++q)
    {
        c.paths += counts[q];
        c.most = std::max<uint32_t>(c.most, counts[q]);
    }
    c.batches = (c.most + c.levels - 1)/c.levels;
    return true;
}

// The batch [t0, t0 + levels): off[q] = the slots in front of pixel q's, off[W*H] = the batch's paths
void samples_offsets(const uint16_t* counts, size_t npix, uint32_t t0, uint32_t levels, std::vector<uint32_t>& off)
{
    off.resize(npix + 1);
    uint32_t sum = 0;
    for (size_t q = 0; q < npix; ++q)
    {
        off[q] = sum;
        sum += counts[q] > t0 ? std::min<uint32_t>(counts[q] - t0, levels) : 0u;
    }
    off[npix] = sum;
}

// The one launch that adds a batch: block t adds the samples its tile's candidates have in the batch (k_samples_accumulate,
// tn_samples.h).  The caller has checked accumulate_tiled_fits.
int launch_samples_accumulate(tinsel_hip* r, hipStream_t st, const FrameParams& fp, float4* rad, float4* target, const uint32_t* passSeeds, const uint32_t* off)
{
    ScopedTimer t(r, KN_ACCUMULATE, st);
    const PathState ps = { rad };
    const int tiles = ((fp.width + kAccTile - 1)/kAccTile)*((fp.height + kAccTile - 1)/kAccTile);
    const int span = 1 + (int)floorf(fp.filterWidth) + (int)ceilf(fp.filterWidth) + 1;     // reachLo + reachHi + 1
    const dim3 grid((unsigned)tiles);
    if (span == 3)
        hipLaunchKernelGGL((k_samples_accumulate<3>), grid, dim3(kBlock), 0, st, ps, fp, target, passSeeds, off);
    else if (span == 4)
        hipLaunchKernelGGL((k_samples_accumulate<4>), grid, dim3(kBlock), 0, st, ps, fp, target, passSeeds, off);
    else
        hipLaunchKernelGGL((k_samples_accumulate<0>), grid, dim3(kBlock), 0, st, ps, fp, target, passSeeds, off);
    HIP_TRY(hipGetLastError());
    return 0;
}

// One batch of a sample-map call on st: the offsets uploaded, its paths generated and traced, its radiance added.  `first`: nothing of
// this call reads the table yet (an earlier call's launches have been waited for by the caller).
int samples_batch(tinsel_hip* r, const BatchPlan& plan, const CameraParams& cam, const FrameParams& fp, uint32_t t0, uint32_t levels,
                  const std::vector<uint32_t>& off, bool first, float4* target, const TraceOverrides& over, hipStream_t st)
{
    const size_t npix = (size_t)fp.width*fp.height;
    const uint32_t n = off[npix];
    if (!n)
        return 0;
    // (the table is one buffer: the batch before this one reads it until its accumulate has run)
    if (!first)
        HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(r->samplesOff.get(), off.data(), sizeof(uint32_t)*(npix + 1), hipMemcpyHostToDevice));

    FrameParams batch = fp;
    batch.passBase = (int)t0;
    batch.numPasses = (int)levels;
    // (the frame of the batch's levels: begin_path splits the slot level*W*H + pixel with it; the paths' own slots are the compact ones)
    if (!batch_frame(r, batch) || (size_t)n >= (size_t)0xffffffffu)
        return fail("render_sample_map: batch too large");
    float4* const rad = (float4*)r->samplesRad.get();
    const SamplesJob job = { r->samplesOff.get(), (uint32_t)npix, n };
    CallerPaths paths;
    paths.samples = &job;
    r->lastLane = 0;
    if (trace_batch(r, plan, r->lane[0], st, &cam, batch, rad, n, &paths, &over))
        return -1;
    return launch_samples_accumulate(r, st, batch, rad, target, r->samplesSeeds.get(), r->samplesOff.get());
}

// Enqueues on st: target[H][W] (device, 16-byte aligned) = AddSample of the samples of levels [0, counts[q]) of every pixel q -- level t
// the path a render starts for q in pass passBegin + t -- from zero or (TINSEL_SAMPLES_ADD) on top of what the plane holds.  Per batch of
// levels (plan_samples under batch_slots) the host's prefix sum makes the compact slot space, k_generate_samples starts the paths in
// front of radiance_pipeline's choice, as a query's are; a finished path writes its radiance to r->samplesRad[its slot], and one
// k_samples_accumulate launch adds them exactly as a render adds a batch's radiance to the accumulator: the call's own seeds for the raster
// positions, options' filter and clamp, a sample that does not exist skipped.  Batches follow each other on st and every pixel's adds stay
// in level order, so the cut shows nowhere.
// Seeds, table, radiance, statistics and fence as views_enqueue (tn_host_views.h); the paths live in the renderer's path buffers, which
// the call takes and leaves as a radiance query does (ensure_batch, batch_fence_wait / own_streams_wait, batch_fence_signal).
int samples_enqueue(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options, uint32_t passBegin, const uint16_t* counts, unsigned flags,
                    float4* target, hipStream_t st)
{
    const size_t npix = (size_t)r->width*r->height;
    const bool add = (flags & TINSEL_SAMPLES_ADD) != 0u;
    const FrameParams fp = frame_params(r, options);

    SamplesCut cut;
    if (!plan_samples(batch_slots(r), fp.width, fp.height, counts, cut))
        return fail("render_sample_map: batch too large");
    if (fp.maxDepth < 1 || cut.most == 0)
    {
        if (!add)
            HIP_TRY(hipMemsetAsync(target, 0, sizeof(float4)*npix, st));        // no bounce or no level, no sample
        return 0;
    }
    const uint32_t levels = (uint32_t)std::min<unsigned long long>(cut.levels, cut.most);

    // (the first batch is the largest: a pixel's share of a batch, clamp(count - t0, 0, levels), does not grow with t0)
    std::vector<uint32_t> off;
    samples_offsets(counts, npix, 0u, levels, off);
    const size_t batchSlots = off[npix];

    // (grown before the first wait on a stream; a buffer that grows may still be read by an earlier call's launches)
    if (query_buffer(r->samplesRad, batchSlots*sizeof(float4)))
        return -1;
    if (r->samplesSeeds.count() < (size_t)cut.most || r->samplesOff.count() < npix + 1)
    {
        if (r->samplesSeeds || r->samplesOff)
            HIP_TRY(hipDeviceSynchronize());
        if (r->samplesSeeds.grow((size_t)cut.most) || r->samplesOff.grow(npix + 1))
            return -1;
    }
    if (!r->samplesStats && r->samplesStats.alloc((size_t)kStatShards*kStatWords))
        return -1;
    if (r->samplesFence.create())
        return -1;
    // (the offsets are uploaded per batch after whatever still reads the last call's)
    if (r->samplesFencePending)
        HIP_TRY(hipEventSynchronize(r->samplesFence));

    CameraParams cam;
    make_camera(*camera, options->width, options->height, cam);

    const BatchPlan plan = plan_batch(r, batchSlots, 1, /*mayOverlap*/ false, PK_GENERATE_SAMPLES);
    if (ensure_batch(r, plan, fp.maxDepth) || batch_fence_wait(r, st) || own_streams_wait(r, st))
        return -1;

    const Rng g = seed_rng_at(r, passBegin);
    hipLaunchKernelGGL(k_pass_seeds, dim3(1), dim3(1), 0, st, g.s1, g.s2, (int)cut.most, r->samplesSeeds.get());
    if (!add)
        HIP_TRY(hipMemsetAsync(target, 0, sizeof(float4)*npix, st));

    TraceOverrides over;
    over.passSeeds = r->samplesSeeds.get();
    over.stats = r->samplesStats.get();

    // (what the renderer remembers of its last batch -- look-ahead's accumulate, the test hooks -- is a render's, not this call's)
    const FrameParams keptFp = r->lastFp;
    const int keptPipeline = r->lastPipeline, keptLane = r->lastLane;
    int rc = 0;
    for (uint32_t t0 = 0; t0 < cut.most && !rc; t0 += levels)
    {
        const uint32_t m = std::min(levels, cut.most - t0);
        if (t0)
            samples_offsets(counts, npix, t0, m, off);
        rc = samples_batch(r, plan, cam, fp, t0, m, off, t0 == 0, target, over, st);
    }
    r->lastFp = keptFp;
    r->lastPipeline = keptPipeline;
    r->lastLane = keptLane;

    // (whatever was enqueued reads the call's buffers and the path buffers: the next user waits for it, failed or not)
    if (hipEventRecord(r->samplesFence, st) == hipSuccess)
    {
        r->samplesFenceStream = st;
        r->samplesFencePending = true;
    }
    if (batch_fence_signal(r, st) || rc)
        return -1;
    HIP_TRY(hipGetLastError());
    return 0;
}

// the refusals of both entries: -1 before anything is written or launched
int samples_args(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options, const uint16_t* counts, unsigned flags, const void* out,
                 const char* who)
{
    const std::string w(who);
    if (!r || !camera || !options || !counts || !out)
        return fail(w + ": null argument");
    if (flags & ~TINSEL_SAMPLES_ADD)
        return fail(w + ": unknown flag bits");
    if (options->mode != TINSEL_MODE_PATHTRACE)
        return fail(w + ": options.mode must be TINSEL_MODE_PATHTRACE");
    if (!r->accum || options->width != r->width || options->height != r->height)
        return fail(w + ": options.width/height do not match the last tinsel_hip_init");
    if ((unsigned long long)r->width*(unsigned long long)r->height >= 0xffffffffull)
        return fail(w + ": W*H must stay below 2^32 - 1");
    if (r->shardWorld > 1)
        return fail(w + ": a sharded renderer (world > 1) has no sample maps");
    if (r->arith != TINSEL_ARITH_EXACT)
        return fail(w + ": the tolerance arithmetic arm (TINSEL_ARITH_FAST) has no sample maps");
    if (!accumulate_tiled_fits(frame_params(r, options)))
        return fail(w + ": the filter's footprint does not fit the tiled accumulate (widths up to 2): there is no untiled masked accumulate kernel");
    return 0;
}

} // namespace

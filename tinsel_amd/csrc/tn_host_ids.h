// tn_host_ids.h -- ID mattes (tinsel_hip_render_id_mattes*): ranked (primitive id, filter-weight sum) lists on the beauty's own samples
// (part of the library's one host translation unit: included by tinsel_hip.hip, in this order, never on its own)
#pragma once

namespace {

// One batch's gather: adds the batch passes [fp.accBegin, fp.accEnd), their ids at `rec`, to the per-pixel lists.  The tiled form where
// the footprint halo fits (accumulate_tiled_fits: filter widths up to 2; a shard: the tiles of its list), else one thread per pixel.
int launch_accumulate_ids(tinsel_hip* r, hipStream_t st, const FrameParams& fp, const int* rec, int* ids, float* weights, const uint32_t* seeds, int slots)
{
    if (!accumulate_tiled_fits(fp))
    {
        hipLaunchKernelGGL(k_ids_accumulate, dim3((unsigned)(((size_t)fp.width*fp.height + kBlock - 1)/kBlock)), dim3(kBlock), 0, st, rec, fp, ids, weights, seeds, slots);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    const bool listed = fp.shardWorld > 1;
    if (listed && accumulate_tile_list(r, fp))
        return -1;
    const int tiles = listed ? r->accTilesCount : ((fp.width + kAccTile - 1)/kAccTile)*((fp.height + kAccTile - 1)/kAccTile);
    if (tiles == 0)
        return 0;               // (a shard without a candidate in the frame: nothing to add)
    const int* const list = listed ? r->accTilesDev.get() : nullptr;
    const int span = 1 + (int)floorf(fp.filterWidth) + (int)ceilf(fp.filterWidth) + 1;     // reachLo + reachHi + 1
    if (span == 3)
        hipLaunchKernelGGL((k_ids_accumulate_tiled<3>), dim3(tiles), dim3(kBlock), 0, st, rec, fp, ids, weights, seeds, list, slots);
    else if (span == 4)
        hipLaunchKernelGGL((k_ids_accumulate_tiled<4>), dim3(tiles), dim3(kBlock), 0, st, rec, fp, ids, weights, seeds, list, slots);
    else
        hipLaunchKernelGGL((k_ids_accumulate_tiled<0>), dim3(tiles), dim3(kBlock), 0, st, rec, fp, ids, weights, seeds, list, slots);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Enqueues on st: the ranked lists of the passes [passBegin, passBegin + passes) into outIds[slots][H][W] and outWeights[slots + 2][H][W]
// (device).  The per-pixel lists start empty (kIdEmpty, weight 0); per batch of whole passes (passes_per_batch, side_pass_batches) k_ids
// writes one 4-byte id per path slot into r->idsRec and one gather adds the batch to the lists in r->idsState; k_ids_rank behind the last
// batch ranks every pixel's list into the caller's buffers.  Batches follow each other on st, every pixel's candidates stay in pass order
// and its slots in first-seen order, so the cut shows nowhere.  Seeds, buffers and fence as features_enqueue (tn_host_features.h), all the
// call's own.
int ids_enqueue(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options, uint32_t passBegin, int passes, int slots, int* outIds,
                float* outWeights, hipStream_t st)
{
    const size_t npix = (size_t)r->width*r->height;

    CameraParams cam;
    make_camera(*camera, options->width, options->height, cam);
    FrameParams fp = frame_params(r, options);

    const size_t perPass = slots_per_pass(r, fp.width, fp.height);
    const int perBatch = passes_per_batch(batch_slots(r), perPass, passes);
    const size_t stride = perPass*(size_t)perBatch;
    if (stride >= (size_t)0xffffffffu)
        return fail("render_id_mattes: batch too large");

    // (grown before the first wait on a stream; a buffer that grows may still be read by an earlier call's launches)
    const size_t idBytes = sizeof(int)*(size_t)kIdMaxSlots*npix, weightBytes = sizeof(float)*(size_t)(kIdMaxSlots + 2)*npix;
    if (query_buffer(r->idsRec, stride*sizeof(int)) || query_buffer(r->idsState, idBytes + weightBytes))
        return -1;
    if (r->idsSeeds.count() < (size_t)passes)
    {
        if (r->idsSeeds)
            HIP_TRY(hipDeviceSynchronize());
        if (r->idsSeeds.alloc((size_t)passes))
            return -1;
    }
    if (r->idsFence.create())
        return -1;
    if (r->idsFencePending && r->idsFenceStream != st)
        HIP_TRY(hipStreamWaitEvent(st, r->idsFence, 0));

    const Rng g = seed_rng_at(r, passBegin);
    hipLaunchKernelGGL(k_pass_seeds, dim3(1), dim3(1), 0, st, g.s1, g.s2, passes, r->idsSeeds.get());
    int* const ids = (int*)r->idsState.get();
    float* const weights = (float*)(r->idsState.get() + idBytes);
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)ids, kIdEmpty, (size_t)kIdMaxSlots*npix, st));
    HIP_TRY(hipMemsetAsync(weights, 0, weightBytes, st));

    int* const rec = (int*)r->idsRec.get();
    int rc = side_pass_batches(r, cam, fp, passes, perBatch, r->idsSeeds.get(), PK_IDS_LDS, PK_IDS, "render_id_mattes",
                               [&](LaunchArgs& a, const FrameParams& batch) {
        a.features.out = rec;
        {
            ScopedTimer t(r, KN_FEATURES, st);
            if (launch_path(r, a, st))
                return -1;
        }
        return launch_accumulate_ids(r, st, batch, rec, ids, weights, r->idsSeeds.get(), slots);
    });
    if (!rc)
        hipLaunchKernelGGL(k_ids_rank, dim3((unsigned)((npix + kBlock - 1)/kBlock)), dim3(kBlock), 0, st, ids, weights, (int)npix, slots, outIds, outWeights);
    // (whatever was enqueued reads the call's buffers: the next call waits for it, failed or not)
    if (hipEventRecord(r->idsFence, st) == hipSuccess)
    {
        r->idsFenceStream = st;
        r->idsFencePending = true;
    }
    if (rc)
        return -1;
    HIP_TRY(hipGetLastError());
    return 0;
}

// the refusals of both entries: -1 before anything is written or launched
int ids_args(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options, int passes, int slots, const void* outIds, const void* outWeights,
             const char* who)
{
    const std::string w(who);
    if (!r || !camera || !options || !outIds || !outWeights)
        return fail(w + ": null argument");
    if (passes < 1)
        return fail(w + ": passes must be >= 1");
    if (slots < 1 || slots > kIdMaxSlots)
        return fail(w + ": slots must be 1 .. TINSEL_ID_MAX_SLOTS");
    if (options->mode != TINSEL_MODE_PATHTRACE)
        return fail(w + ": options.mode must be TINSEL_MODE_PATHTRACE");
    if (!r->accum || options->width != r->width || options->height != r->height)
        return fail(w + ": options.width/height do not match the last tinsel_hip_init");
    return 0;
}

} // namespace

// tn_host_api.h -- C-ABI: init / render / present / settings / statistics / test hooks / scene packs
// (part of the library's one host translation unit: included by tinsel_hip.hip, in this order, never on its own)
#pragma once

extern "C" {

int tinsel_hip_init(tinsel_hip* r, int width, int height)
{
    if (r)
        lookahead_release(r);
    if (!r || width <= 0 || height <= 0)
        return fail("init: bad arguments");
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipDeviceSynchronize());
    r->accum = nullptr;
    if (r->accumOwn.alloc((size_t)width*height))
        return -1;
    r->accum = r->accumOwn.get();
    HIP_TRY(hipMemset(r->accum, 0, sizeof(float4)*(size_t)width*height));
    HIP_TRY(hipStreamSynchronize(nullptr));     // before anything is accumulated on another (non-blocking) stream: see ensure_batch
    r->width = width;
    r->height = height;
    return 0;
}

int tinsel_hip_init_external(tinsel_hip* r, int width, int height, float* device_accum)
{
    if (r)
        lookahead_release(r);
    if (!r || width <= 0 || height <= 0 || !device_accum)
        return fail("init_external: bad arguments");
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipDeviceSynchronize());
    r->accumOwn.reset();
    r->accum = (float4*)device_accum;       // the caller's: a view, never freed here
    HIP_TRY(hipMemset(r->accum, 0, sizeof(float4)*(size_t)width*height));
    HIP_TRY(hipStreamSynchronize(nullptr));
    r->width = width;
    r->height = height;
    return 0;
}

int tinsel_hip_render_async(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options, int passes, void* stream)
{
    lookahead_cancel(r);
    return render_impl(r, camera, options, passes, (hipStream_t)stream);
}

int tinsel_hip_set_lookahead(tinsel_hip* r, int enable)
{
    if (!r)
        return fail("set_lookahead: null");
    if (!enable)
        lookahead_cancel(r);
    if (enable != TINSEL_LOOKAHEAD_PIN_OUTPUT && r->pinned.held())
    {
        (void)hipSetDevice(r->device);
        r->pinned.release(r->copyStream);
    }
    r->lookahead = enable == TINSEL_LOOKAHEAD_PIN_OUTPUT ? TINSEL_LOOKAHEAD_PIN_OUTPUT : (enable ? TINSEL_LOOKAHEAD_ON : TINSEL_LOOKAHEAD_OFF);
    return 0;
}

int tinsel_hip_render(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options, float* out_rgba, int passes)
{
    if (r && r->lookahead && out_rgba && camera && options && r->accum && r->accumOwn && passes >= 1 &&
        options->width == r->width && options->height == r->height)
        return lookahead_render(r, camera, options, out_rgba, passes);
    lookahead_cancel(r);
    if (render_impl(r, camera, options, passes, nullptr))
        return -1;
    if (out_rgba)
        return tinsel_hip_read_accum(r, out_rgba);
    HIP_TRY(hipStreamSynchronize(nullptr));
    return 0;
}

int tinsel_hip_render_cost(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options, uint32_t pass_begin, int passes,
                           uint32_t* out_host)
{
    lookahead_cancel(r);
    return render_cost_impl(r, camera, options, pass_begin, passes, out_host);
}

// Ray queries (tn_query.h, tn_host_query.h).  Nothing of the renderer's state is written and look-ahead work in flight is left alone: a query
// only reads the scene, like the kernels that may be running beside it.
static int query_args(tinsel_hip* r, int mode, long long n, const void* rays, const void* out, const char* who)
{
    if (!r || !rays || !out || n < 0 || n > 0x7fffffffll || (mode != TINSEL_QUERY_CLOSEST && mode != TINSEL_QUERY_OCCLUDED))
        return fail(std::string(who) + ": bad arguments (a renderer, TINSEL_QUERY_CLOSEST or TINSEL_QUERY_OCCLUDED, 0 <= n < 2^31, two arrays)");
    return 0;
}

int tinsel_hip_trace_rays_device(tinsel_hip* r, int mode, long long n, const tinsel_ray* rays_dev, void* out_dev, void* stream)
{
    if (query_args(r, mode, n, rays_dev, out_dev, "trace_rays_device"))
        return -1;
    const size_t outStride = mode == TINSEL_QUERY_CLOSEST ? sizeof(tinsel_ray_hit) : sizeof(uint32_t);
    if (query_arrays({ { rays_dev, (size_t)n*sizeof(tinsel_ray) }, { out_dev, (size_t)n*outStride } }, "trace_rays_device") ||
        query_ready(r, "trace_rays_device"))
        return -1;
    if (n == 0)
        return 0;
    return launch_query(r, mode, (size_t)n, rays_dev, out_dev, nullptr, 0, 0.0f, (hipStream_t)stream);
}

int tinsel_hip_trace_rays(tinsel_hip* r, int mode, long long n, const tinsel_ray* rays_host, void* out_host)
{
    if (query_args(r, mode, n, rays_host, out_host, "trace_rays") || query_ready(r, "trace_rays"))
        return -1;
    const size_t outStride = mode == TINSEL_QUERY_CLOSEST ? sizeof(tinsel_ray_hit) : sizeof(uint32_t);
    return staged_chunks((size_t)n, std::min<size_t>((size_t)n, kQueryChunk), { rays_host, &r->queryRaysDev, sizeof(tinsel_ray) },
                         { out_host, &r->queryOutDev, outStride }, {}, [&](size_t, size_t m) {
        return launch_query(r, mode, m, r->queryRaysDev.get(), r->queryOutDev.get(), nullptr, 0, 0.0f, nullptr);
    });
}

int tinsel_hip_trace_camera(tinsel_hip* r, const tinsel_camera* camera, int width, int height, float time, tinsel_ray_hit* out_host)
{
    if (!r || !camera || !out_host || width <= 0 || height <= 0 || (long long)width*height > 0x7fffffffll)
        return fail("trace_camera: bad arguments (a renderer, a camera, a positive frame size, an array of width*height records)");
    if (query_ready(r, "trace_camera"))
        return -1;
    const size_t n = (size_t)width*height;
    CameraParams cam;
    make_camera(*camera, width, height, cam);
    return staged_chunks(n, std::min(n, kQueryCameraChunk), {}, { out_host, &r->queryOutDev, sizeof(tinsel_ray_hit) }, {}, [&](size_t done, size_t m) {
        return launch_query(r, kQueryCamera, m, nullptr, r->queryOutDev.get(), &cam, width, time, nullptr, (uint32_t)done);
    });
}

// Radiance queries (tn_radiance.h, tn_host_radiance.h): the integrator on paths the caller starts.  The accumulator, the pass index, the pass
// seeds and the tuning are not touched, look-ahead work in flight is waited for on the device and kept; rays and samples are counted.
int tinsel_hip_trace_radiance_device(tinsel_hip* r, long long n, const tinsel_path_start* starts_dev, int max_depth, float* out_rgbx_dev, void* stream)
{
    if (radiance_args(r, n, starts_dev, out_rgbx_dev, max_depth, "trace_radiance_device"))
        return -1;
    if (query_arrays({ { starts_dev, (size_t)n*sizeof(tinsel_path_start) }, { out_rgbx_dev, (size_t)n*sizeof(float4) } }, "trace_radiance_device") ||
        query_ready(r, "trace_radiance_device"))
        return -1;
    if (n == 0)
        return 0;
    return trace_radiance(r, (size_t)n, starts_dev, (float4*)out_rgbx_dev, max_depth, (hipStream_t)stream);
}

int tinsel_hip_trace_radiance(tinsel_hip* r, long long n, const tinsel_path_start* starts_host, int max_depth, float* out_rgbx_host)
{
    if (radiance_args(r, n, starts_host, out_rgbx_host, max_depth, "trace_radiance") || query_ready(r, "trace_radiance"))
        return -1;
    return staged_chunks((size_t)n, std::min<size_t>((size_t)n, kRadianceChunk), { starts_host, &r->queryRaysDev, sizeof(tinsel_path_start) },
                         { out_rgbx_host, &r->queryOutDev, sizeof(float4) }, {}, [&](size_t, size_t m) {
        return trace_radiance(r, m, r->queryRaysDev.get(), (float4*)r->queryOutDev.get(), max_depth, nullptr);
    });
}

// Gather queries (tn_gather.h, tn_host_gather.h): `samples` paths from each point, drawn on the device, one mean per point -- or, for the SH
// entries, the (order + 1)^2 coefficients of bands 0 .. order per point (k_gather_sh_reduce behind the same batches).  As radiance
// queries: nothing of the renderer's frame state is touched, rays and samples are counted.
// (order: kGatherMean or, judged by gather_sh_order in the SH entries before they come here, 0 .. 2)
static int gather_device(tinsel_hip* r, int mode, int order, long long n, const tinsel_gather_point* points_dev, int samples, int max_depth, float* out_dev,
                         tinsel_path_start* starts_out_dev, void* stream, const char* who)
{
    if (gather_args(r, mode, n, points_dev, samples, max_depth, out_dev, who))
        return -1;
    if (query_arrays({ { points_dev, (size_t)n*sizeof(tinsel_gather_point) }, { out_dev, (size_t)n*gather_out_each(order)*sizeof(float4) },
                       { starts_out_dev, starts_out_dev ? (size_t)n*(size_t)samples*sizeof(tinsel_path_start) : 0 } }, who) ||
        query_ready(r, who))
        return -1;
    if (n == 0)
        return 0;
    return trace_gather(r, mode, order, (size_t)n, points_dev, samples, max_depth, (float4*)out_dev, starts_out_dev, (hipStream_t)stream);
}

static int gather_host(tinsel_hip* r, int mode, int order, long long n, const tinsel_gather_point* points_host, int samples, int max_depth, float* out_host,
                       tinsel_path_start* starts_out_host, const char* who)
{
    if (gather_args(r, mode, n, points_host, samples, max_depth, out_host, who) || query_ready(r, who))
        return -1;
    const size_t each = gather_out_each(order);
    return staged_chunks((size_t)n, gather_chunk((size_t)n, samples, starts_out_host != nullptr, each), { points_host, &r->queryRaysDev, sizeof(tinsel_gather_point) },
                         { out_host, &r->queryOutDev, sizeof(float4)*each }, { starts_out_host, &r->gatherStartsDev, sizeof(tinsel_path_start)*(size_t)samples },
                         [&](size_t, size_t m) {
        return trace_gather(r, mode, order, m, r->queryRaysDev.get(), samples, max_depth, (float4*)r->queryOutDev.get(),
                            starts_out_host ? r->gatherStartsDev.get() : nullptr, nullptr);
    });
}

int tinsel_hip_gather_radiance_device(tinsel_hip* r, int mode, long long n, const tinsel_gather_point* points_dev, int samples, int max_depth,
                                      float* out_rgbx_dev, tinsel_path_start* starts_out_dev, void* stream)
{
    return gather_device(r, mode, kGatherMean, n, points_dev, samples, max_depth, out_rgbx_dev, starts_out_dev, stream, "gather_radiance_device");
}

int tinsel_hip_gather_radiance(tinsel_hip* r, int mode, long long n, const tinsel_gather_point* points_host, int samples, int max_depth,
                               float* out_rgbx_host, tinsel_path_start* starts_out_host)
{
    return gather_host(r, mode, kGatherMean, n, points_host, samples, max_depth, out_rgbx_host, starts_out_host, "gather_radiance");
}

int tinsel_hip_gather_sh_device(tinsel_hip* r, int mode, int order, long long n, const tinsel_gather_point* points_dev, int samples, int max_depth,
                                float* out_dev, tinsel_path_start* starts_out_dev, void* stream)
{
    return gather_sh_order(order, "gather_sh_device") ? -1 :
           gather_device(r, mode, order, n, points_dev, samples, max_depth, out_dev, starts_out_dev, stream, "gather_sh_device");
}

int tinsel_hip_gather_sh(tinsel_hip* r, int mode, int order, long long n, const tinsel_gather_point* points_host, int samples, int max_depth,
                         float* out_host, tinsel_path_start* starts_out_host)
{
    return gather_sh_order(order, "gather_sh") ? -1 : gather_host(r, mode, order, n, points_host, samples, max_depth, out_host, starts_out_host, "gather_sh");
}

// Feature buffers (tn_features.h, tn_host_features.h): the first-hit albedo, normal and depth of the camera's own paths, reconstructed as the
// beauty is.  Own seeds, own buffers: nothing of the renderer's frame state is written, look-ahead work in flight is left alone, no statistics.
int tinsel_hip_render_features_device(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options, uint32_t pass_begin, int passes,
                                      unsigned features, float* out_dev, void* stream)
{
    if (features_args(r, camera, options, passes, features, out_dev, "render_features_device"))
        return -1;
    if (query_arrays({ { out_dev, (size_t)r->width*r->height*sizeof(float4)*(size_t)__builtin_popcount(features) } }, "render_features_device") ||
        query_ready(r, "render_features_device"))
        return -1;
    return features_enqueue(r, camera, options, pass_begin, passes, features, (float4*)out_dev, (hipStream_t)stream);
}

int tinsel_hip_render_features(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options, uint32_t pass_begin, int passes,
                               unsigned features, float* out_host)
{
    if (features_args(r, camera, options, passes, features, out_host, "render_features") || query_ready(r, "render_features"))
        return -1;
    const size_t bytes = (size_t)r->width*r->height*sizeof(float4)*(size_t)__builtin_popcount(features);
    if (query_buffer(r->featOut, bytes) || features_enqueue(r, camera, options, pass_begin, passes, features, (float4*)r->featOut.get(), nullptr))
        return -1;
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(hipMemcpy(out_host, r->featOut.get(), bytes, hipMemcpyDeviceToHost));
    return 0;
}

// ID mattes (tn_ids.h, tn_host_ids.h): per pixel a ranked list of (primitive id, filter-weight sum) pairs over the camera's own paths.  Own
// seeds, own buffers, as the feature buffers; the gather and the ranking have no class in tinsel_hip_kernel_times.
int tinsel_hip_render_id_mattes_device(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options, uint32_t pass_begin, int passes,
                                       int slots, int32_t* out_ids_dev, float* out_weights_dev, void* stream)
{
    const char* const who = "render_id_mattes_device";
    if (ids_args(r, camera, options, passes, slots, out_ids_dev, out_weights_dev, who))
        return -1;
    const size_t npix = (size_t)r->width*r->height;
    if (query_arrays({ { out_ids_dev, npix*sizeof(int32_t)*(size_t)slots }, { out_weights_dev, npix*sizeof(float)*(size_t)(slots + 2) } }, who) ||
        query_ready(r, who))
        return -1;
    return ids_enqueue(r, camera, options, pass_begin, passes, slots, out_ids_dev, out_weights_dev, (hipStream_t)stream);
}

int tinsel_hip_render_id_mattes(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options, uint32_t pass_begin, int passes,
                                int slots, int32_t* out_ids_host, float* out_weights_host)
{
    const char* const who = "render_id_mattes";
    if (ids_args(r, camera, options, passes, slots, out_ids_host, out_weights_host, who) || query_ready(r, who))
        return -1;
    const size_t npix = (size_t)r->width*r->height;
    const size_t idBytes = npix*sizeof(int32_t)*(size_t)slots, weightBytes = npix*sizeof(float)*(size_t)(slots + 2);
    if (query_buffer(r->idsOut, idBytes + weightBytes))
        return -1;
    int* const ids = (int*)r->idsOut.get();
    float* const weights = (float*)(r->idsOut.get() + idBytes);
    if (ids_enqueue(r, camera, options, pass_begin, passes, slots, ids, weights, nullptr))
        return -1;
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(hipMemcpy(out_ids_host, ids, idBytes, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_weights_host, weights, weightBytes, hipMemcpyDeviceToHost));
    return 0;
}

// Light groups (tn_split.h k_shade_groups, tn_host_light_groups.h): the beauty split per emitter group in one trace of the camera's paths
// through the split pipeline.  Own seeds, own planes, own statistics block: nothing of the renderer's frame state is written; the path
// buffers are used under the radiance queries' fences, look-ahead work in flight is waited for on the device and kept.
int tinsel_hip_render_light_groups_device(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options, uint32_t pass_begin, int passes,
                                          int num_groups, const int32_t* group_of_primitive, int env_group, float* out_dev, void* stream)
{
    const char* const who = "render_light_groups_device";
    if (light_groups_args(r, camera, options, passes, num_groups, group_of_primitive, env_group, out_dev, who))
        return -1;
    if (query_arrays({ { out_dev, (size_t)r->width*r->height*sizeof(float4)*(size_t)num_groups } }, who) || query_ready(r, who))
        return -1;
    return light_groups_enqueue(r, camera, options, pass_begin, passes, num_groups, group_of_primitive, env_group, (float4*)out_dev, (hipStream_t)stream);
}

int tinsel_hip_render_light_groups(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options, uint32_t pass_begin, int passes,
                                   int num_groups, const int32_t* group_of_primitive, int env_group, float* out_host)
{
    const char* const who = "render_light_groups";
    if (light_groups_args(r, camera, options, passes, num_groups, group_of_primitive, env_group, out_host, who) || query_ready(r, who))
        return -1;
    const size_t bytes = (size_t)r->width*r->height*sizeof(float4)*(size_t)num_groups;
    if (query_buffer(r->groupsOut, bytes) ||
        light_groups_enqueue(r, camera, options, pass_begin, passes, num_groups, group_of_primitive, env_group, (float4*)r->groupsOut.get(), nullptr))
        return -1;
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(hipMemcpy(out_host, r->groupsOut.get(), bytes, hipMemcpyDeviceToHost));
    return 0;
}

// Depth planes (tn_split.h k_shade_depths, tn_host_depth_planes.h): the beauty at several path depths in one trace of the camera's paths
// through the split pipeline.  Own seeds, own planes, own statistics block: nothing of the renderer's frame state is written; the path
// buffers are used under the radiance queries' fences, look-ahead work in flight is waited for on the device and kept.
int tinsel_hip_render_depth_planes_device(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options, uint32_t pass_begin, int passes,
                                          int num_planes, const int32_t* depths, int flags, float* out_dev, void* stream)
{
    const char* const who = "render_depth_planes_device";
    if (depth_planes_args(r, camera, options, passes, num_planes, depths, flags, out_dev, who))
        return -1;
    if (query_arrays({ { out_dev, (size_t)r->width*r->height*sizeof(float4)*(size_t)num_planes } }, who) || query_ready(r, who))
        return -1;
    return depth_planes_enqueue(r, camera, options, pass_begin, passes, num_planes, depths, flags, (float4*)out_dev, (hipStream_t)stream);
}

int tinsel_hip_render_depth_planes(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options, uint32_t pass_begin, int passes,
                                   int num_planes, const int32_t* depths, int flags, float* out_host)
{
    const char* const who = "render_depth_planes";
    if (depth_planes_args(r, camera, options, passes, num_planes, depths, flags, out_host, who) || query_ready(r, who))
        return -1;
    const size_t bytes = (size_t)r->width*r->height*sizeof(float4)*(size_t)num_planes;
    if (query_buffer(r->depthsOut, bytes))
        return -1;
    // (the staging planes are the host entry's alone, and it returns when they have been read: nothing in flight touches them)
    if (flags & TINSEL_DEPTH_PLANES_ADD)
        HIP_TRY(hipMemcpy(r->depthsOut.get(), out_host, bytes, hipMemcpyHostToDevice));
    if (depth_planes_enqueue(r, camera, options, pass_begin, passes, num_planes, depths, flags, (float4*)r->depthsOut.get(), nullptr))
        return -1;
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(hipMemcpy(out_host, r->depthsOut.get(), bytes, hipMemcpyDeviceToHost));
    return 0;
}

// View batches (tn_views.h, tn_host_views.h): the frames of many cameras in one call, k_generate_views in front of a radiance query's
// pipeline and one accumulate launch per batch of views behind it.  Own seeds, own radiance, own statistics block: nothing of the
// renderer's frame state is written; the path buffers are used under the radiance queries' fences, look-ahead work in flight is waited for
// on the device and kept.
int tinsel_hip_render_views_device(tinsel_hip* r, const tinsel_camera* cameras, int num_views, const tinsel_options* options, uint32_t pass_begin,
                                   int passes, unsigned flags, float* out_rgba_dev, void* stream)
{
    const char* const who = "render_views_device";
    if (views_args(r, cameras, num_views, options, passes, flags, out_rgba_dev, who))
        return -1;
    if (query_arrays({ { out_rgba_dev, (size_t)r->width*r->height*sizeof(float4)*(size_t)num_views } }, who) || query_ready(r, who))
        return -1;
    return views_enqueue(r, cameras, num_views, options, pass_begin, passes, flags, (float4*)out_rgba_dev, (hipStream_t)stream);
}

int tinsel_hip_render_views(tinsel_hip* r, const tinsel_camera* cameras, int num_views, const tinsel_options* options, uint32_t pass_begin,
                            int passes, unsigned flags, float* out_rgba_host)
{
    const char* const who = "render_views";
    if (views_args(r, cameras, num_views, options, passes, flags, out_rgba_host, who) || query_ready(r, who))
        return -1;
    const size_t bytes = (size_t)r->width*r->height*sizeof(float4)*(size_t)num_views;
    // (TINSEL_VIEWS_ADD without a bounce leaves the planes untouched: nothing to carry to the device and back)
    if ((flags & TINSEL_VIEWS_ADD) && options->max_depth < 1)
        return 0;
    if (query_buffer(r->viewsOut, bytes))
        return -1;
    // (the staging planes are the host entry's alone, and it returns when they have been read: nothing in flight touches them)
    if (flags & TINSEL_VIEWS_ADD)
        HIP_TRY(hipMemcpy(r->viewsOut.get(), out_rgba_host, bytes, hipMemcpyHostToDevice));
    if (views_enqueue(r, cameras, num_views, options, pass_begin, passes, flags, (float4*)r->viewsOut.get(), nullptr))
        return -1;
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(hipMemcpy(out_rgba_host, r->viewsOut.get(), bytes, hipMemcpyDeviceToHost));
    return 0;
}

int tinsel_hip_plan_views(unsigned long long slot_limit, int width, int height, int passes, int num_views, int* out3)
{
    if (!out3 || width < 1 || height < 1 || passes < 1 || num_views < 1)
        return fail("plan_views: bad arguments");
    ViewsCut c;
    if (!plan_views((size_t)slot_limit, width, height, passes, num_views, c))
        return fail("plan_views: a batch would not fit the 32-bit slot index");
    out3[0] = c.viewsPerBatch;
    out3[1] = c.passesPerBatch;
    out3[2] = (int)std::min<long long>(c.batches, 0x7fffffffll);
    return 0;
}

// Sample maps (tn_samples.h, tn_host_samples.h): a per-pixel pass count in one call, k_generate_samples on compact slots in front of a
// radiance query's pipeline and one masked accumulate launch per batch of levels behind it.  Own seeds, own radiance, own statistics
// block, as a views call: nothing of the renderer's frame state is written.
int tinsel_hip_render_sample_map_device(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options, uint32_t pass_begin,
                                        const uint16_t* counts, unsigned flags, float* out_rgba_dev, void* stream)
{
    const char* const who = "render_sample_map_device";
    if (samples_args(r, camera, options, counts, flags, out_rgba_dev, who))
        return -1;
    if (query_arrays({ { out_rgba_dev, (size_t)r->width*r->height*sizeof(float4) } }, who) || query_ready(r, who))
        return -1;
    return samples_enqueue(r, camera, options, pass_begin, counts, flags, (float4*)out_rgba_dev, (hipStream_t)stream);
}

int tinsel_hip_render_sample_map(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options, uint32_t pass_begin,
                                 const uint16_t* counts, unsigned flags, float* out_rgba_host)
{
    const char* const who = "render_sample_map";
    if (samples_args(r, camera, options, counts, flags, out_rgba_host, who) || query_ready(r, who))
        return -1;
    const size_t npix = (size_t)r->width*r->height, bytes = npix*sizeof(float4);
    // (nothing to trace: the plane is zeroed, or with TINSEL_SAMPLES_ADD left untouched, without a trip to the device)
    if (options->max_depth < 1 || std::all_of(counts, counts + npix, [](uint16_t c) { return c == 0; }))
    {
        if (!(flags & TINSEL_SAMPLES_ADD))
            memset(out_rgba_host, 0, bytes);
        return 0;
    }
    if (query_buffer(r->samplesOut, bytes))
        return -1;
    // (the staging plane is the host entry's alone, and it returns when it has been read: nothing in flight touches it)
    if (flags & TINSEL_SAMPLES_ADD)
        HIP_TRY(hipMemcpy(r->samplesOut.get(), out_rgba_host, bytes, hipMemcpyHostToDevice));
    if (samples_enqueue(r, camera, options, pass_begin, counts, flags, (float4*)r->samplesOut.get(), nullptr))
        return -1;
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(hipMemcpy(out_rgba_host, r->samplesOut.get(), bytes, hipMemcpyDeviceToHost));
    return 0;
}

int tinsel_hip_plan_sample_map(unsigned long long slot_limit, int width, int height, const uint16_t* counts, unsigned long long* out4)
{
    if (!out4 || !counts || width < 1 || height < 1)
        return fail("plan_sample_map: bad arguments");
    SamplesCut c;
    if (!plan_samples(slot_limit, width, height, counts, c))
        return fail("plan_sample_map: a batch would not fit the 32-bit slot index");
    out4[0] = c.levels;
    out4[1] = c.batches;
    out4[2] = c.paths;
    out4[3] = c.most;
    return 0;
}

float* tinsel_hip_accum_device_ptr(tinsel_hip* r) { return r ? (float*)r->accum : nullptr; }

int tinsel_hip_read_accum(tinsel_hip* r, float* out_rgba)
{
    if (!r || !r->accum || !out_rgba)
        return fail("read_accum: bad arguments");
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out_rgba, r->accum, sizeof(float4)*(size_t)r->width*r->height, hipMemcpyDeviceToHost));
    return 0;
}

// The feature-guided denoise stage (tn_denoise.h, tn_host_denoise.h): a joint non-local-means filter on linear radiance.  Own buffers:
// nothing of the renderer's frame state is written, no statistics, no class in tinsel_hip_kernel_times.
void tinsel_hip_denoise_params_init(tinsel_hip_denoise_params* p)
{
    if (p)
        *p = denoise_defaults();
}

int tinsel_hip_denoise_device(tinsel_hip* r, const float* beauty_dev, const float* planes_dev, unsigned features, int width, int height,
                              const tinsel_hip_denoise_params* p, float* out_dev, void* stream)
{
    const char* const who = "denoise_device";
    if (denoise_args(r, planes_dev, features, width, height, p, out_dev, who))
        return -1;
    if ((((uintptr_t)beauty_dev | (uintptr_t)planes_dev | (uintptr_t)out_dev) & 15u) != 0)
        return fail(std::string(who) + ": the arrays must be 16-byte aligned");
    if (!beauty_dev && denoise_own_beauty(r, width, height, who))
        return -1;
    HIP_TRY(hipSetDevice(r->device));
    return denoise_enqueue(r, beauty_dev ? (const float4*)beauty_dev : r->accum, (const float4*)planes_dev, features, width, height, p, (float4*)out_dev,
                           (hipStream_t)stream);
}

int tinsel_hip_denoise(tinsel_hip* r, const float* beauty_host, const float* planes_host, unsigned features, int width, int height,
                       const tinsel_hip_denoise_params* p, float* out_host)
{
    const char* const who = "denoise";
    if (denoise_args(r, planes_host, features, width, height, p, out_host, who))
        return -1;
    if (!beauty_host && denoise_own_beauty(r, width, height, who))
        return -1;
    HIP_TRY(hipSetDevice(r->device));
    const size_t image = sizeof(float4)*(size_t)width*height;
    const size_t planes = image*(size_t)__builtin_popcount(features);
    // [beauty][planes] on the device; the accumulator is read where it is
    if (query_buffer(r->denoiseIn, image + planes) || query_buffer(r->denoiseOut, image))
        return -1;
    unsigned char* const in = r->denoiseIn.get();
    if (beauty_host)
        HIP_TRY(hipMemcpy(in, beauty_host, image, hipMemcpyHostToDevice));
    else
        HIP_TRY(hipDeviceSynchronize());        // (as tinsel_hip_read_accum: whatever still adds to the accumulator)
    if (planes)
        HIP_TRY(hipMemcpy(in + image, planes_host, planes, hipMemcpyHostToDevice));
    if (denoise_enqueue(r, beauty_host ? (const float4*)in : r->accum, (const float4*)(in + image), features, width, height, p, (float4*)r->denoiseOut.get(),
                        nullptr))
        return -1;
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(hipMemcpy(out_host, r->denoiseOut.get(), image, hipMemcpyDeviceToHost));
    return 0;
}

// The display stage of the reference's frame loop (main.cpp:258-282) on an accumulator-form image of the init size.
static int present_enqueue(tinsel_hip* r, const float4* source, const tinsel_options* options, int nlm_width, float nlm_falloff, hipStream_t st)
{
    HIP_TRY(hipSetDevice(r->device));
    const size_t n = (size_t)r->width*r->height;
    if (options->mode != TINSEL_MODE_PATHTRACE)
    {
        r->presented = source;          // main.cpp:258: the other modes present the raw pixels
        return 0;
    }
    if (r->display[0].count() != n)
    {
        HIP_TRY(hipDeviceSynchronize());
        for (DevBuf<float4>& d : r->display)
            d.reset();
    }
    const int needed = nlm_width ? 3 : 1;
    for (int i = 0; i < needed; ++i)
        if (r->display[i].grow(n))
            return -1;
    float4* const display[3] = { r->display[0].get(), r->display[1].get(), r->display[2].get() };

    {
        ScopedTimer t(r, KN_PRESENT, st);
        hipLaunchKernelGGL(k_present, dim3((unsigned)((n + 255)/256)), dim3(256), 0, st, source, display[0], (int)n,
                           options->exposure, options->limit);
    }
    r->presented = display[0];
    if (nlm_width)
    {
        const dim3 grid((r->width + 15)/16, (r->height + 15)/16);
        {
            ScopedTimer t(r, KN_NLM_MEANS, st);
            hipLaunchKernelGGL(k_nlm_means, grid, dim3(256), 0, st, display[0], display[1], r->width, r->height, nlm_width);
        }
        {
            ScopedTimer t(r, KN_NLM, st);
            hipLaunchKernelGGL(k_nlm, grid, dim3(256), 0, st, display[0], display[1], display[2], r->width, r->height,
                               nlm_falloff, nlm_width);
        }
        r->presented = display[2];
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int tinsel_hip_present_image_device(tinsel_hip* r, const float* image_dev, const tinsel_options* options, int nlm_width, float nlm_falloff, void* stream)
{
    if (!r || !image_dev || !options || nlm_width < 0)
        return fail("present_image_device: bad arguments");
    if (((uintptr_t)image_dev & 15u) != 0)
        return fail("present_image_device: the image must be 16-byte aligned");
    if (!r->accum)
        return fail("present_image_device: no tinsel_hip_init (the image has the init size)");
    return present_enqueue(r, (const float4*)image_dev, options, nlm_width, nlm_falloff, (hipStream_t)stream);
}

// ... on the device accumulator
int tinsel_hip_present_async(tinsel_hip* r, const tinsel_options* options, int nlm_width, float nlm_falloff, void* stream)
{
    if (!r || !r->accum || !options || nlm_width < 0)
        return fail("present: bad arguments (Init and Render first)");
    return tinsel_hip_present_image_device(r, (const float*)r->accum, options, nlm_width, nlm_falloff, stream);
}

int tinsel_hip_present(tinsel_hip* r, const tinsel_options* options, int nlm_width, float nlm_falloff, float* out_rgba)
{
    if (tinsel_hip_present_async(r, options, nlm_width, nlm_falloff, nullptr))
        return -1;
    HIP_TRY(hipStreamSynchronize(nullptr));
    if (out_rgba)
        HIP_TRY(hipMemcpy(out_rgba, r->presented, sizeof(float4)*(size_t)r->width*r->height, hipMemcpyDeviceToHost));
    return 0;
}

const float* tinsel_hip_present_device_ptr(tinsel_hip* r) { return r ? (const float*)r->presented : nullptr; }

// WritePng's 8-bit quantisation (png.cpp:323-343): one serial default-seeded Random stream dithers every
// channel (two Randf per channel), all in double until the narrowing at the Quantize(float) call.  Host code:
// the generator is a nonlinear recurrence (no skip-ahead), 6 draws per pixel.
int tinsel_image_quantize_rgb8(const float* rgba, int width, int height, unsigned char* rgb)
{
    if (!rgba || !rgb || width <= 0 || height <= 0)
        return fail("quantize: bad arguments");
    Rng rand = Rng::seeded(0u);
    const size_t n = (size_t)width*height;
    for (size_t i = 0; i < n; ++i)
    {
        for (int c = 0; c < 3; ++c)
        {
            const double a = (double)rgba[i*4 + c]*255.0;
            const float r1 = rand.randf();
            const float r2 = rand.randf();
            const float x = (float)(((a + (double)r1) + (double)r2) - (double)0.5f);
            // Clamp = Min(Max(x, 0), 255) with Max(a,b) = (a < b) ? b : a, Min(a,b) = (a < b) ? a : b  (maths.h:55-64)
            const float lo = (x < 0.0f) ? 0.0f : x;
            const float cl = (lo < 255.0f) ? lo : 255.0f;
            rgb[i*3 + c] = (unsigned char)(int)cl;
        }
    }
    return 0;
}

// Probe importance sampling: the reference's two binary searches (default, sample-identical) or an alias table.
int tinsel_hip_set_probe_sampling(tinsel_hip* r, int mode)
{
    lookahead_cancel(r);
    if (!r || (mode != TINSEL_PROBE_CDF && mode != TINSEL_PROBE_ALIAS))
        return fail("set_probe_sampling: bad arguments");
    if (mode == TINSEL_PROBE_CDF || !r->scene.probe.valid)
    {
        r->scene.probe.alias = nullptr;
        return 0;
    }
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipDeviceSynchronize());
    if (!r->probeAlias)
    {
        // Vose's alias method over p(row, col) = pdfY[row]*pdfX[row, col] -- the probabilities ProbeSample's two searches
        // realise (probe.h:31-79 BuildCDF) -- in double on the host, once
        const int W = r->scene.probe.width, H = r->scene.probe.height;
        const size_t n = (size_t)W*H;
        std::vector<float> px(n), py((size_t)H);
        HIP_TRY(hipMemcpy(px.data(), r->scene.probe.pdfX, sizeof(float)*n, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(py.data(), r->scene.probe.pdfY, sizeof(float)*(size_t)H, hipMemcpyDeviceToHost));
        std::vector<double> scaled(n);
        double total = 0.0;
        for (int j = 0; j < H; ++j)
            for (int i = 0; i < W; ++i)
            {
                // a row with pdfY == 0 has probability 0 whatever its pdfX holds: BuildCDF leaves 0*inf = NaN there for an all-black row,
                // and 0*NaN would make the total NaN
                const double p = (py[(size_t)j] == 0.0f) ? 0.0 : (double)py[(size_t)j]*(double)px[(size_t)j*W + i];
                scaled[(size_t)j*W + i] = p;
                total += p;
            }
        if (!(total > 0.0))
            return fail("set_probe_sampling: the probe has no energy");
        std::vector<uint32_t> small, large;
        small.reserve(n); large.reserve(n);
        for (size_t k = 0; k < n; ++k)
        {
            scaled[k] = scaled[k]/total*(double)n;
            (scaled[k] < 1.0 ? small : large).push_back((uint32_t)k);
        }
        std::vector<uint2> table(n);
        while (!small.empty() && !large.empty())
        {
            const uint32_t s = small.back(); small.pop_back();
            const uint32_t l = large.back();
            const float keep = (float)scaled[s];
            table[s] = make_uint2(__builtin_bit_cast(uint32_t, keep), l);
            scaled[l] = (scaled[l] + scaled[s]) - 1.0;
            if (scaled[l] < 1.0)
            {
                large.pop_back();
                small.push_back(l);
            }
        }
        const float one = 2.0f;         // r2 <= 1 < 2: always keep
        for (uint32_t k : large) table[k] = make_uint2(__builtin_bit_cast(uint32_t, one), k);
        for (uint32_t k : small) table[k] = make_uint2(__builtin_bit_cast(uint32_t, one), k);
        DevBuf<uint2> alias;
        if (alias.upload(table.data(), n))
            return -1;
        r->probeAlias = std::move(alias);
    }
    r->scene.probe.alias = r->probeAlias.get();
    return 0;
}

int tinsel_hip_set_russian_roulette(tinsel_hip* r, int start_bounce)
{
    lookahead_cancel(r);
    if (!r || start_bounce < 0)
        return fail("set_russian_roulette: bad arguments");
    r->rrStart = start_bounce;
    return 0;
}

int tinsel_hip_write_accum(tinsel_hip* r, const float* rgba, uint32_t next_pass_index)
{
    lookahead_cancel(r);
    if (!r || !r->accum || !rgba)
        return fail("write_accum: bad arguments (Init first)");
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(r->accum, rgba, sizeof(float4)*(size_t)r->width*r->height, hipMemcpyHostToDevice));
    r->passIndex = next_pass_index;
    return 0;
}

int tinsel_hip_set_shard(tinsel_hip* r, int rank, int world, int tile)
{
    lookahead_cancel(r);
    if (!r || world < 1 || rank < 0 || rank >= world || tile < 1)
        return fail("set_shard: bad arguments");
    if (rank != r->shardRank || world != r->shardWorld || tile != r->shardTile)
    {
        HIP_TRY(hipSetDevice(r->device));
        HIP_TRY(hipDeviceSynchronize());
        free_batch(r);          // ownership changes: start from clean path buffers
    }
    r->shardRank = rank;
    r->shardWorld = world;
    r->shardTile = tile;
    return 0;
}

int tinsel_hip_set_arithmetic(tinsel_hip* r, int mode)
{
    lookahead_cancel(r);
    if (!r || (mode != TINSEL_ARITH_EXACT && mode != TINSEL_ARITH_FAST))
        return fail("set_arithmetic: bad arguments");
    if (tinsel_fast_launch_args_size() != sizeof(LaunchArgs))
        return fail("set_arithmetic: the two builds of the path kernels disagree on the launch record");
    r->arith = mode;
    return 0;
}

int tinsel_hip_get_arithmetic(tinsel_hip* r) { return r ? r->arith : TINSEL_ARITH_EXACT; }

int tinsel_hip_set_pipeline(tinsel_hip* r, int pipeline)
{
    lookahead_cancel(r);
    if (!r || pipeline < TINSEL_PIPELINE_WAVEFRONT || pipeline > TINSEL_PIPELINE_WAVEFRONT_PAIRED)
        return fail("set_pipeline: bad arguments");
    r->pipeline = pipeline;
    return 0;
}

int tinsel_hip_set_pass_index(tinsel_hip* r, uint32_t pass_index)
{
    lookahead_cancel(r);
    if (!r)
        return fail("set_pass_index: null");
    r->passIndex = pass_index;
    return 0;
}

uint32_t tinsel_hip_get_pass_index(tinsel_hip* r) { return r ? r->passIndex : 0; }

static int read_stats(tinsel_hip* r, unsigned long long* out8)
{
    std::vector<unsigned long long> shards((size_t)kStatShards*kStatWords);
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(shards.data(), r->statsDev.get(), sizeof(unsigned long long)*shards.size(), hipMemcpyDeviceToHost));
    for (int w = 0; w < kStatWords; ++w)
        out8[w] = 0;
    for (int b = 0; b < kStatShards; ++b)
        for (int w = 0; w < kStatWords; ++w)
            out8[w] += shards[(size_t)b*kStatWords + w];
    return 0;
}

void tinsel_hip_stats(tinsel_hip* r, unsigned long long* rays, unsigned long long* samples, double* gpu_seconds)
{
    unsigned long long s[8] = { 0 };
    if (r && r->statsDev)
        (void)read_stats(r, s);
    if (rays) *rays = s[0];
    if (samples) *samples = s[1];
    if (gpu_seconds) *gpu_seconds = r ? r->gpuSeconds : 0.0;
}

/* extended counters: [0]=rays [1]=samples [2]=internal node visits [3]=triangle tests
 * [4]=primitive tests [5]=shadow rays ; [2..4] only count while detail counting is on */
int tinsel_hip_stats_detail(tinsel_hip* r, unsigned long long* out8)
{
    if (!r || !out8)
        return fail("stats_detail: bad arguments");
    return read_stats(r, out8);
}

int tinsel_hip_set_detail_counters(tinsel_hip* r, int enable)
{
    lookahead_cancel(r);
    if (!r)
        return fail("set_detail_counters: null");
    r->countDetail = enable != 0;
    return 0;
}

void tinsel_hip_reset_stats(tinsel_hip* r)
{
    lookahead_cancel(r);
    if (!r)
        return;
    (void)hipSetDevice(r->device);
    (void)hipDeviceSynchronize();
    (void)hipMemset(r->statsDev.get(), 0, sizeof(unsigned long long)*kStatShards*kStatWords);
    (void)hipStreamSynchronize(nullptr);
    r->gpuSeconds = 0.0;
}

int tinsel_hip_enable_kernel_timing(tinsel_hip* r, int enable)
{
    lookahead_cancel(r);
    if (!r)
        return fail("enable_kernel_timing: null");
    r->timing = enable != 0;
    return 0;
}

int tinsel_hip_kernel_time_bytes(void) { return (int)sizeof(tinsel_kernel_time); }

int tinsel_hip_kernel_times(tinsel_hip* r, tinsel_kernel_time* out, int max_entries)
{
    lookahead_cancel(r);
    if (!r || !out)
        return fail("kernel_times: bad arguments");
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipDeviceSynchronize());
    float total[KN_COUNT] = { 0 };
    uint32_t launches[KN_COUNT] = { 0 };
    // busy time: the union of a kernel's launch intervals -- launches of one kernel on two streams overlap (render_impl's chunks), and
    // the sum of their durations counts the shared stretch twice
    std::vector<std::pair<float, float>> intervals[KN_COUNT];
    for (const TimedSpan& s : r->spans)
    {
        float ms = 0.0f, at = 0.0f;
        if (hipEventElapsedTime(&ms, s.start, s.stop) == hipSuccess)
        {
            total[s.kernel] += ms;
            launches[s.kernel]++;
            if (hipEventElapsedTime(&at, r->spans.front().start, s.start) == hipSuccess)
                intervals[s.kernel].push_back(std::make_pair(at, at + ms));
        }
    }
    float busy[KN_COUNT] = { 0 };
    for (int k = 0; k < KN_COUNT; ++k)
    {
        std::sort(intervals[k].begin(), intervals[k].end());
        float end = -1e30f;
        for (const auto& iv : intervals[k])
        {
            if (iv.second > end)
                busy[k] += iv.second - std::max(iv.first, end);
            end = std::max(end, iv.second);
        }
        if (intervals[k].size() != launches[k])
            busy[k] = total[k];
    }
    int n = 0;
    double sum = 0.0;
    for (int k = 0; k < KN_COUNT && n < max_entries; ++k)
    {
        if (!launches[k])
            continue;
        memset(&out[n], 0, sizeof(out[n]));
        strncpy(out[n].name, kKernelNames[k], sizeof(out[n].name) - 1);
        out[n].launches = launches[k];
        out[n].total_ms = total[k];
        out[n].busy_ms = busy[k];
        sum += total[k];
        ++n;
    }
    r->gpuSeconds += sum*1e-3;
    return n;
}

int tinsel_hip_reserve(tinsel_hip* r, int passes, int max_depth)
{
    lookahead_cancel(r);
    if (!r || !r->accum || passes < 1 || max_depth < 1)
        return fail("reserve: bad arguments (Init first)");
    HIP_TRY(hipSetDevice(r->device));
    const size_t perPass = slots_per_pass(r, r->width, r->height);
    return ensure_batch(r, plan_batch(r, perPass, passes_per_batch(batch_slots(r), perPass, passes), /*mayOverlap*/ false), max_depth);
}

int tinsel_hip_set_batch_paths(tinsel_hip* r, unsigned long long max_paths)
{
    lookahead_cancel(r);
    if (!r || max_paths < 1024)
        return fail("set_batch_paths: bad arguments");
    r->maxBatchSlots = (size_t)max_paths;
    r->batchSlotsExplicit = true;
    r->tune.batch_paths = (int64_t)max_paths;
    return 0;
}

// The per-render fields of the tuning (include/tinsel_hip.h): the create-time ones are baked into the uploaded scene and stay as created.
int tinsel_hip_set_tuning(tinsel_hip* r, const tinsel_hip_tuning* tuning)
{
    if (!r || !tuning)
        return fail("set_tuning: null argument");
    lookahead_cancel(r);
    tinsel_hip_tuning t = tuning_from_caller(tuning);
    if (t.grid_mult < 0 || t.grid_mult > 256 || (t.walk_block != 0 && t.walk_block != 256 && t.walk_block != 1024) ||
        t.accumulate < TINSEL_ACCUMULATE_AUTO || t.accumulate > TINSEL_ACCUMULATE_FULL_WINDOW || t.walk_refill_min > 64 || t.walk_leaf_min > 64 || t.walk_grid_mult < 0 || t.walk_grid_mult > 64 ||
        (t.tail_split > 0 && (!(t.tail_share >= 0.0f) || t.tail_divide < 1)) || (t.batch_paths != 0 && t.batch_paths < 1024))
        return fail("set_tuning: a field is out of range");
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipDeviceSynchronize());        // (launches in flight use the path buffers free_batch gives back)
    const tinsel_hip_tuning was = r->tune;
    t.flat_scan = was.flat_scan; t.lds_scene = was.lds_scene; t.walk = was.walk; t.inline_max_tris = was.inline_max_tris;
    t.walk_min_tris = was.walk_min_tris; t.small_mesh_bytes = was.small_mesh_bytes; t.arena_lds_limit = was.arena_lds_limit;
    r->tune = t;
    if (t.batch_paths > 0)
    {
        r->maxBatchSlots = (size_t)t.batch_paths;
        r->batchSlotsExplicit = true;
    }
    else
    {
        r->maxBatchSlots = 8u << 20;
        r->batchSlotsExplicit = false;
    }
    free_batch(r);          // (the region arrays are sized by grid_mult)
    if (pairs_planes(r, was) != pairs_planes(r, t) && !r->planeTablePrims.empty())
    {
        // the plane table once more, with or without its pairs: the scene level in force, derived again
        SceneLevel lvl;
        if (!build_scene_level(r->sceneBvhHost, r->primsHost, r->planeTablePrims, pairs_planes(r, t), lvl))
            return fail("set_tuning: the scene level could not be derived again");
        return upload_scene_level(r, lvl);
    }
    return 0;
}

int tinsel_hip_get_tuning(tinsel_hip* r, tinsel_hip_tuning* out)
{
    if (!r || !out)
        return fail("get_tuning: null argument");
    *out = r->tune;
    return 0;
}

long long tinsel_hip_read_batch_radiance(tinsel_hip* r, float* out_rgbx, unsigned long long max_paths)
{
    lookahead_cancel(r);
    if (!r || !out_rgbx)
        return fail("read_batch_radiance: bad arguments");
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipDeviceSynchronize());
    const size_t n = std::min<size_t>((size_t)max_paths, r->lastBatchSlots);
    if (n)
        HIP_TRY(hipMemcpy(out_rgbx, r->ps.rad, sizeof(float4)*n, hipMemcpyDeviceToHost));
    return (long long)n;
}

int tinsel_hip_leaf(tinsel_hip* r, int op, int index, int n, const float* in, int in_stride, const uint32_t* seeds,
                    float* out, int out_stride, const tinsel_camera* camera, int width, int height)
{
    lookahead_cancel(r);
    if (!r || n <= 0 || !out || out_stride <= 0 || op < 0 || op > kLeafDisplay)
        return fail("leaf: bad arguments");
    if ((op == kLeafBsdfEval || op == kLeafBsdfSample || op == kLeafPrimIntersect || op == kLeafPrimSample) &&
        (index < 0 || index >= r->scene.numPrims))
        return fail("leaf: primitive index out of range");
    if (r->arith == TINSEL_ARITH_FAST && tinsel_fast_leaf_args_size() != sizeof(LeafArgs))
        return fail("leaf: the two builds of k_leaf disagree on the argument record");
    HIP_TRY(hipSetDevice(r->device));
    DevBuf<float> dIn, dOut;
    DevBuf<uint32_t> dSeeds;
    CameraParams cam;
    memset(&cam, 0, sizeof(cam));
    if (camera && width > 0 && height > 0)
        make_camera(*camera, width, height, cam);
    if (in && in_stride > 0 && dIn.upload(in, (size_t)n*in_stride))
        return fail("leaf: input upload failed");
    if (seeds && dSeeds.upload(seeds, (size_t)n))
        return fail("leaf: seed upload failed");
    if (dOut.alloc((size_t)n*out_stride))
        return fail("leaf: output allocation failed");
    LeafArgs a;
    memset(&a, 0, sizeof(a));
    a.scene = r->scene;
    a.op = op; a.index = index; a.n = n;
    a.in = dIn.get(); a.inStride = in_stride;
    a.seeds = dSeeds.get();
    a.out = dOut.get(); a.outStride = out_stride;
    a.cam = cam;
    a.stackEntries = r->stackNeed;
    a.ldsBytes = (uint32_t)stack_bytes(r);
    // the renderer's arm (tinsel_hip_set_arithmetic): this translation unit's k_leaf, or the tolerance build's
    if (r->arith == TINSEL_ARITH_FAST)
        tinsel_fast_launch_leaf(&a, nullptr);
    else
        launch_leaf(a, nullptr);
    if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess)
        return fail("leaf: kernel failed");
    if (hipMemcpy(out, dOut.get(), sizeof(float)*(size_t)n*out_stride, hipMemcpyDeviceToHost) != hipSuccess)
        return fail("leaf: download failed");
    return 0;
}

int tinsel_hip_stack_entries(tinsel_hip* r) { return r ? r->stackNeed : 0; }

int tinsel_hip_mesh_tree(tinsel_hip* r, int primitive, void* out_nodes, int capacity, int* out_meta)
{
    lookahead_cancel(r);
    if (!r || !out_meta || capacity < 0 || primitive < 0 || primitive >= r->scene.numPrims || r->primMesh[(size_t)primitive] < 0)
        return fail("mesh_tree: bad arguments (a mesh primitive and a meta array of 7 ints)");
    const DevMesh& dm = r->meshesNow[(size_t)r->primMesh[(size_t)primitive]];
    const int meta[7] = { (int)dm.root, dm.numInternal, dm.numTris, dm.stackNeed, dm.topCount, dm.twoLeaves, dm.inArena };
    memcpy(out_meta, meta, sizeof(meta));
    if (!out_nodes)
        return dm.numInternal;
    if (capacity < dm.numInternal)
        return fail("mesh_tree: capacity is smaller than the tree's node count");
    // an arena mesh's tree as every launch stages it: the arena's copy in HBM
    const unsigned char* src = dm.inArena ? r->scene.arena + dm.offNodes : reinterpret_cast<const unsigned char*>(dm.nodes);
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipDeviceSynchronize());
    if (dm.numInternal > 0)
        HIP_TRY(hipMemcpy(out_nodes, src, sizeof(Node64)*(size_t)dm.numInternal, hipMemcpyDeviceToHost));
    return dm.numInternal;
}
int tinsel_hip_walked_prims(tinsel_hip* r) { return (r && r->walkEnabled) ? r->walkPrims.count : 0; }
int tinsel_hip_nee_per_path(tinsel_hip* r) { return r ? r->neePerPath : 0; }

int tinsel_hip_walk_tops(tinsel_hip* r, int* out_counts, int capacity)
{
    if (!r || !out_counts || capacity < 0)
        return fail("walk_tops: bad arguments");
    const int n = r->walkEnabled ? r->walkPrims.count : 0;
    if (capacity < n)
        return fail("walk_tops: capacity is smaller than the number of walked primitives");
    // (plan_walk reads the scene and the tuning in force: what the next render's k_walk launches stage)
    const WalkPlan w = plan_walk(r);
    for (int k = 0; k < n; ++k)
        out_counts[k] = w.job.topCount[k];
    return n;
}

unsigned int tinsel_hip_scene_features(const tinsel_scene_desc* scene)
{
    if (!scene || !scene->primitives)
        return 0u;
    uint32_t f = scene->probe_valid ? kFeatProbe : 0u;
    for (int i = 0; i < scene->num_primitives; ++i)
    {
        const tinsel_primitive& p = scene->primitives[i];
        const tinsel_material& m = p.material;
        f |= (m.absorption.x != 0.0f || m.absorption.y != 0.0f || m.absorption.z != 0.0f) ? kFeatMedia : 0u;
        f |= m.transmission != 0.0f ? kFeatTransmission : 0u;
        f |= memcmp(&p.start_transform, &p.end_transform, sizeof(tinsel_transform)) != 0 ? kFeatMotion : 0u;
        f |= p.type == TINSEL_GEOM_SPHERE ? kFeatSphere : 0u;
        if (p.type == TINSEL_GEOM_MESH)
        {
            // one internal node over two leaves (a quad) is tested without the stack walk (DevMesh::twoLeaves, ray_mesh_two_leaves)
            const tinsel_bvh_node* n = p.geo.mesh.nodes;
            const bool twoLeaves = n && p.geo.mesh.num_nodes == 3 && !ref_is_leaf(n[0]) && n[0].left_index < 3u && ref_right(n[0]) < 3u &&
                                   ref_is_leaf(n[n[0].left_index]) && ref_is_leaf(n[ref_right(n[0])]);
            f |= twoLeaves ? 0u : kFeatMeshWalk;
        }
    }
    return f;
}

int tinsel_hip_scene_plane_pairs(const tinsel_scene_desc* scene, int32_t* out_pairs, int capacity, int* out_singles)
{
    if (out_singles)
        *out_singles = 0;
    if (!scene || !scene->primitives || !scene->bvh_nodes || capacity < 0)
        return 0;
    // the planes create would put into the table: those whose leaf of the scene BVH is an "infinite" box
    std::vector<int32_t> planes;
    std::vector<float> eqs;
    for (int n = 0; n < scene->num_bvh_nodes; ++n)
    {
        const tinsel_bvh_node& nd = scene->bvh_nodes[n];
        if (!ref_is_leaf(nd) || nd.left_index >= (uint32_t)scene->num_primitives || scene->primitives[nd.left_index].type != TINSEL_GEOM_PLANE)
            continue;
        if (make_prim_box(nd).alwaysHit && std::find(planes.begin(), planes.end(), (int32_t)nd.left_index) == planes.end())
            planes.push_back((int32_t)nd.left_index);
    }
    std::sort(planes.begin(), planes.end());
    for (const int32_t k : planes)
        eqs.insert(eqs.end(), scene->primitives[k].geo.plane.plane, scene->primitives[k].geo.plane.plane + 4);
    const std::vector<std::pair<int, int>> pairs = pair_planes(eqs);
    for (size_t q = 0; q < pairs.size() && out_pairs && (int)q < capacity; ++q)
    {
        out_pairs[2*q] = planes[(size_t)pairs[q].first];
        out_pairs[2*q + 1] = planes[(size_t)pairs[q].second];
    }
    if (out_singles)
        *out_singles = (int)planes.size() - 2*(int)pairs.size();
    return (int)pairs.size();
}

int tinsel_hip_plane_table(tinsel_hip* r, int* out2)
{
    if (!r || !out2)
        return fail("plane_table: bad arguments");
    out2[0] = r->planePairs;
    out2[1] = r->planeSingles;
    return 0;
}

int tinsel_hip_scene_slim(const tinsel_scene_desc* scene)
{
    if (!scene || !scene->primitives)
        return 0;
    bool anySubsurface = false;
    for (int i = 0; i < scene->num_primitives; ++i)
        anySubsurface = anySubsurface || !is_plus_zero(scene->primitives[i].material.subsurface);
    return scene_slim(tinsel_hip_scene_features(scene), anySubsurface) ? 1 : 0;
}

int tinsel_hip_bounce_plan(tinsel_hip* r, uint32_t* out2)
{
    if (!r || !out2)
        return fail("bounce_plan: bad arguments");
    if (r->lastBounceKind < 0)
        return fail("bounce_plan: the fused kernel has not run yet");
    out2[0] = (uint32_t)r->lastBounceKind;
    out2[1] = r->lastBounceFeatures;
    return 0;
}

long long tinsel_hip_bake_source(tinsel_hip* r, char* out_text, unsigned long long capacity, char* out_key65, int* out_bakeable)
{
    if (!r)
        return fail("bake_source: null renderer");
    return bake_source_of(r, out_text, capacity, out_key65, out_bakeable);
}

int tinsel_hip_install_baked(tinsel_hip* r, const void* image, unsigned long long bytes, const char* key, int how)
{
    if (!r)
        return fail("install_baked: null renderer");
    if (!image && how == TINSEL_BAKE_NO_COMPILER)
    {
        if (!r->baked.fn)
            r->baked.how = how;
        return 0;
    }
    if (!image || bytes < 64 || !key || strlen(key) != 64 || (how != TINSEL_BAKE_COMPILED && how != TINSEL_BAKE_FROM_CACHE))
        return fail("install_baked: bad arguments (a code object, its 64-digit key, TINSEL_BAKE_COMPILED or _FROM_CACHE)");
    lookahead_cancel(r);
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipDeviceSynchronize());            // (a launch in flight may be running the module this one replaces)
    Module fresh;
    if (fresh.load(image))
        return -1;
    hipFunction_t fn = nullptr;
    HIP_TRY(hipModuleGetFunction(&fn, fresh, kBakedKernelName));
    // the raised dynamic-LDS limit of the library's own instance (prepare_path_kernels); where the runtime has no such attribute for a
    // module's function, the instance serves the launches that stay within the default limit
    uint32_t ldsLimit = 65536;
    if (hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, r->sharedMemLimit) == hipSuccess)
        ldsLimit = (uint32_t)r->sharedMemLimit;
    else
        (void)hipGetLastError();
    r->baked.module = std::move(fresh);
    r->baked.fn = fn;
    r->baked.key = key;
    r->baked.how = how;
    r->baked.ldsLimit = ldsLimit;
    r->baked.launches = 0;
    return 0;
}

int tinsel_hip_set_bounce_bake(tinsel_hip* r, int mode)
{
    if (!r || mode < -1 || mode > 1)
        return fail("set_bounce_bake: bad arguments (-1 auto, 0 never, 1 always)");
    lookahead_cancel(r);
    r->baked.mode = mode;
    return 0;
}

int tinsel_hip_get_bounce_bake(tinsel_hip* r) { return r ? r->baked.mode : -1; }

int tinsel_hip_bake_status(tinsel_hip* r, uint32_t* out3, char* out_key65)
{
    if (!r || !out3)
        return fail("bake_status: bad arguments");
    if (out_key65)
        memcpy(out_key65, r->baked.fn ? r->baked.key.c_str() : "", r->baked.fn ? 65 : 1);
    out3[1] = (uint32_t)(r->baked.launches & 0xffffffffull);
    out3[2] = (uint32_t)(r->baked.launches >> 32);
    if (r->baked.mode == 0)
        out3[0] = TINSEL_BAKE_OFF;
    else if (!plans_fit_closed(r, nullptr))
        out3[0] = TINSEL_BAKE_NOT_BAKEABLE;
    else if (!r->baked.fn)
        out3[0] = r->baked.how == TINSEL_BAKE_NO_COMPILER ? TINSEL_BAKE_NO_COMPILER : TINSEL_BAKE_NONE;
    else
        // (a closed launch asks for the traversal stacks and the staged arena, no pools: stack_bytes)
        out3[0] = r->baked.key != bake_live_key(r) ? (uint32_t)TINSEL_BAKE_STALE :
                  stack_bytes(r) > (size_t)r->baked.ldsLimit ? (uint32_t)TINSEL_BAKE_LDS_REFUSED : (uint32_t)r->baked.how;
    return 0;
}

int tinsel_hip_queue_counts(tinsel_hip* r, uint32_t* out, int max_bounces)
{
    if (!r || !out || max_bounces < 1)
        return fail("queue_counts: bad arguments");
    if (r->batchPipeline < 0 || r->batchDepth < 1)
        return fail("queue_counts: nothing rendered yet");
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipDeviceSynchronize());
    const int n = std::min(max_bounces, std::min(r->batchDepth, r->lastFp.maxDepth));
    if (r->lastPipeline == TINSEL_PIPELINE_MEGAKERNEL || r->batchPipeline != r->lastPipeline)
        return fail("queue_counts: the last batch did not run a wavefront pipeline");
    // the counts are kept per region, in the lane of the chunk traced last
    const tinsel_hip::DenseLane& lane = r->lane[r->lastLane];
    const bool split = r->lastPipeline == TINSEL_PIPELINE_WAVEFRONT_SPLIT && r->neePerPath > 0;
    const size_t W = lane.regions;
    std::vector<uint32_t> seg(W*(size_t)n*4, 0u);
    uint32_t* const src[4] = { lane.ss.segFront, lane.ss.segBack, lane.ss.neeFront, lane.ss.neeBack };
    for (int a = 0; a < (split ? 4 : 2); ++a)
        HIP_TRY(hipMemcpy(seg.data() + (size_t)a*W*n, src[a], W*(size_t)n*sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (int b = 0; b < n; ++b)
    {
        unsigned long long live = 0, nee = 0;
        for (size_t g = 0; g < W; ++g)
        {
            live += seg[(size_t)b*W + g] + seg[W*n + (size_t)b*W + g];
            nee += seg[2*W*n + (size_t)b*W + g] + seg[3*W*n + (size_t)b*W + g];
        }
        // the fused kernel generates bounce 0's paths itself
        out[b] = (b == 0 && r->lastPipeline == TINSEL_PIPELINE_WAVEFRONT) ? lane.paths : (uint32_t)live;
        out[max_bounces + b] = (uint32_t)nee;
    }
    return n;
}

// ---------------------------------------------------------------------------
// scene packs

// Yard-sticks on this GPU (tn_ubench.h): kind 0 = float4 stream copy of `bytes` bytes (units = bytes read + written),
// kinds 1..3 = dependent 64-B record chases through a table of `bytes` bytes rounded down to a power of two, `steps` visits
// per lane (units = records visited); the kind only names the kernel for the profiler (1 beyond the Infinity Cache, 2 the size
// of a walked tree, 3 inside one L2).  One warm-up launch, then one timed with HIP events.
// How a batch of `slots` path slots would be cut into regions on a device of `num_cus` CUs (streaming_grid + cut_regions): pure host
// arithmetic, no device needed -- tests/test_abi.py checks its invariants over the whole range of batch sizes on the CPU box
int tinsel_hip_plan_regions(unsigned long long slots, int num_cus, int nee_per_path, int fused, unsigned int* out)
{
    if (!out || slots == 0 || slots >= 0xffffffffull || num_cus < 1 || num_cus > 4096)
        return fail("plan_regions: bad arguments");
    // (the default tuning; alloc_dense's region arrays, positions for the batch + a wave per region)
    RegionSpec s = region_spec(tuning_defaults(), num_cus, nee_per_path, fused != 0, kBounceWaves);
    s.capacity = (size_t)slots + s.maxRegions*kWave;
    RegionCut c;
    const int rc = cut_regions(s, (size_t)slots, streaming_grid(s, (size_t)slots), c) ? 0 : fail("render: path buffers too small for this batch");
    out[0] = c.numRegions; out[1] = c.regionLen; out[2] = c.bigRegions; out[3] = c.shortLen;
    out[4] = (unsigned int)c.grid(); out[5] = (unsigned int)s.maxRegions;
    return rc;
}

int tinsel_hip_selftest_arith(int device_index, int op, int variant, unsigned long long* out_counts, unsigned int* out_first_bad)
{
    if (!out_counts || !out_first_bad || op < 0 || op > 2)
        return fail("selftest_arith: bad arguments");
    if (variant < 0)
        variant = op == 0 ? kRcpVariant : op == 1 ? kSqrtVariant : kRsqrtVariant;      // what this library is built with
    HIP_TRY(hipSetDevice(device_index));
    DevBuf<unsigned long long> countsDev;
    DevBuf<uint32_t> firstDev;
    if (countsDev.alloc(260))
        return -1;
    if (firstDev.alloc(1))
        return fail("selftest_arith: allocation failed");
    unsigned long long* const counts = countsDev.get();
    uint32_t* const first = firstDev.get();
    (void)hipMemset(counts, 0, 260*sizeof(unsigned long long));
    (void)hipMemset(first, 0xff, sizeof(uint32_t));
    bool known = true;
    switch (op*100 + variant)
    {
    case 0: launch_selftest_arith<0, 0>(counts, first); break;
    case 1: launch_selftest_arith<0, 1>(counts, first); break;
    case 11: launch_selftest_arith<0, 11>(counts, first); break;
    case 100: launch_selftest_arith<1, 0>(counts, first); break;
    case 101: launch_selftest_arith<1, 1>(counts, first); break;
    case 111: launch_selftest_arith<1, 11>(counts, first); break;
    case 121: launch_selftest_arith<1, 21>(counts, first); break;
    case 200: launch_selftest_arith<2, 0>(counts, first); break;
    case 201: launch_selftest_arith<2, 1>(counts, first); break;
    case 202: launch_selftest_arith<2, 2>(counts, first); break;
    case 203: launch_selftest_arith<2, 3>(counts, first); break;
    default: known = false; break;
    }
    if (!known)
        return fail("selftest_arith: unknown variant");
    if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess ||
             hipMemcpy(out_counts, counts, 260*sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess ||
             hipMemcpy(out_first_bad, first, sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)
        return fail("selftest_arith: kernel failed");
    return 0;
}

// The library's own sort and scan (tn_sort.h: the device BVH builder's) on caller data: keys[0, n) sorted in place by their bits
// [begin_bit, end_bit) (multiples of 8), keys with equal bits keeping their order; out[i] = in[0] + .. + in[i - 1].
int tinsel_hip_selftest_sort(int device_index, unsigned long long* keys, unsigned long long n, int begin_bit, int end_bit)
{
    if (!keys || n == 0 || n >= (1ull << 31) || begin_bit < 0 || end_bit > 64 || begin_bit >= end_bit || (begin_bit & 7) || (end_bit & 7))
        return fail("selftest_sort: bad arguments");
    HIP_TRY(hipSetDevice(device_index));
    DevBuf<unsigned long long> a, b;
    DevBuf<int> scratch;
    if (a.alloc((size_t)n) || b.alloc((size_t)n) || scratch.alloc(sort_scratch_ints((size_t)n)))
        return fail("selftest_sort: allocation failed");
    if (hipMemcpy(a.get(), keys, n*8, hipMemcpyHostToDevice) != hipSuccess)
        return fail("selftest_sort: upload failed");
    radix_sort_keys(a.get(), b.get(), (size_t)n, begin_bit, end_bit, scratch.get(), nullptr);
    if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess || hipMemcpy(keys, b.get(), n*8, hipMemcpyDeviceToHost) != hipSuccess)
        return fail("selftest_sort: kernels failed");
    return 0;
}

int tinsel_hip_selftest_scan(int device_index, const int* in, int* out, unsigned long long n)
{
    if (!in || !out || n == 0 || n >= (1ull << 31))
        return fail("selftest_scan: bad arguments");
    HIP_TRY(hipSetDevice(device_index));
    DevBuf<int> a, scratch;
    if (a.alloc((size_t)n) || scratch.alloc(scan_scratch_ints((size_t)n)))
        return fail("selftest_scan: allocation failed");
    if (hipMemcpy(a.get(), in, n*sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
        return fail("selftest_scan: upload failed");
    exclusive_scan(a.get(), a.get(), (size_t)n, scratch.get(), nullptr);         // (in place, as the builder's radix passes use it)
    if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess || hipMemcpy(out, a.get(), n*sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
        return fail("selftest_scan: kernels failed");
    return 0;
}

// launch_accumulate's rule (accumulate_support_rule), for callers and tests: host arithmetic only
int tinsel_hip_accumulate_support(int filter_type, float filter_width, float filter_falloff, float filter_offset, float* out_arg_zero)
{
    float z = 0.0f;
    const bool takes = accumulate_support_rule(filter_type, filter_width, filter_falloff, filter_offset, &z);
    if (out_arg_zero)
        *out_arg_zero = z;
    return takes ? 1 : 0;
}

// The accumulate stage on caller data: radiance[passes][height][width] (rgbx) added to accum[height][width] (rgba) by exactly the launch
// launch_accumulate makes for such a frame on this device (one shard).  choice: tinsel_hip_tuning::accumulate; form 0: as the library
// decides, 1: the full window, 2: the support form (an error where the filter or the chosen kernel has none).  *out_form: what ran.
int tinsel_hip_selftest_accumulate(int device_index, int width, int height, int filter_type, float filter_width, float filter_falloff, float filter_offset,
                                   float clamp, const unsigned int* pass_seeds, int passes, const float* radiance, float* accum, int choice, int form,
                                   int* out_form)
{
    if (width < 1 || height < 1 || passes < 1 || !pass_seeds || !radiance || !accum || !out_form || form < 0 || form > 2 ||
        choice < TINSEL_ACCUMULATE_AUTO || choice > TINSEL_ACCUMULATE_FULL_WINDOW || (size_t)width*height*passes >= ((size_t)1 << 31))
        return fail("selftest_accumulate: bad arguments");
    HIP_TRY(hipSetDevice(device_index));
    int numCUs = 0;
    HIP_TRY(hipDeviceGetAttribute(&numCUs, hipDeviceAttributeMultiprocessorCount, device_index));
    const size_t npix = (size_t)width*height;
    FrameParams fp = {};                    // (frame_params + batch_frame for one unsharded batch of `passes` passes)
    fp.width = width;
    fp.height = height;
    fp.npixM = 0xffffffffu/(uint32_t)npix;
    fp.widthM = 0xffffffffu/(uint32_t)width;
    fp.shardRank = 0; fp.shardWorld = 1; fp.shardTile = 32;
    fp.shardPerPass = (uint32_t)npix;
    fp.filterType = filter_type;
    fp.filterWidth = filter_width;
    fp.filterFalloff = filter_falloff;
    fp.filterOffset = filter_offset;
    fp.clampLen = clamp;
    fp.passBase = 0;
    fp.numPasses = passes;
    fp.accBegin = 0;
    fp.accEnd = passes;
    DevBuf<float4> rad, acc;
    DevBuf<uint32_t> seeds;
    if (rad.alloc(npix*passes) || acc.alloc(npix) || seeds.alloc((size_t)passes))
        return fail("selftest_accumulate: allocation failed");
    if (hipMemcpy(rad.get(), radiance, npix*passes*sizeof(float4), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(acc.get(), accum, npix*sizeof(float4), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(seeds.get(), pass_seeds, (size_t)passes*sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess)
        return fail("selftest_accumulate: upload failed");
    const int ran = launch_accumulate_kernels(numCUs, choice, form != 1, seeds.get(), nullptr, -1, nullptr, fp, rad.get(), acc.get());
    if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess || hipMemcpy(accum, acc.get(), npix*sizeof(float4), hipMemcpyDeviceToHost) != hipSuccess)
        return fail("selftest_accumulate: kernel failed");
    *out_form = ran;
    if (form == 2 && ran != ACC_FORM_SUPPORT_TILED && ran != ACC_FORM_SUPPORT_WIDE)
        return fail("selftest_accumulate: no support form for this filter and kernel choice");
    return 0;
}

int tinsel_hip_ubench(int device_index, int kind, unsigned long long bytes, int steps, double* out_ms, double* out_units)
{
    if (kind < 0 || kind > 3 || bytes < 4096 || !out_ms || !out_units)
        return fail("ubench: bad arguments");
    HIP_TRY(hipSetDevice(device_index));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device_index));
    Event e0, e1;
    if (e0.create(true) || e1.create(true))
        return -1;
    float ms = 0.0f;
    int rc = 0;
    if (kind == 0)
    {
        const size_t n = (size_t)bytes/sizeof(float4);
        DevBuf<float4> inDev, outDev;
        float4* const in = inDev.alloc(n) ? nullptr : inDev.get();
        float4* const out = outDev.alloc(n) ? nullptr : outDev.get();
        if (!in || !out || hipMemset(in, 0x3c, n*sizeof(float4)) != hipSuccess)
            rc = fail("ubench: allocation failed");
        else
        {
            // the best of a few shapes (workgroups per CU x interleaved / workgroup-contiguous x plain / non-temporal): what this chip sustains, not what one shape gets
            float best = 0.0f;
            for (int shape = 0; shape < 12 && !rc; ++shape)
            {
                const unsigned grid = (unsigned)prop.multiProcessorCount*(shape % 3 == 0 ? 8u : shape % 3 == 1 ? 16u : 32u);
                const bool contig = (shape/3) % 2 == 1 && n % ((size_t)grid*256*8) == 0;
                auto launch = [&] {
                    if (shape < 6)
                    {
                        if (contig) hipLaunchKernelGGL((k_ub_copy<false, true>), dim3(grid), dim3(256), 0, nullptr, (const float4*)in, out, n);
                        else hipLaunchKernelGGL((k_ub_copy<false, false>), dim3(grid), dim3(256), 0, nullptr, (const float4*)in, out, n);
                    }
                    else
                    {
                        if (contig) hipLaunchKernelGGL((k_ub_copy<true, true>), dim3(grid), dim3(256), 0, nullptr, (const float4*)in, out, n);
                        else hipLaunchKernelGGL((k_ub_copy<true, false>), dim3(grid), dim3(256), 0, nullptr, (const float4*)in, out, n);
                    }
                };
                launch();
                (void)hipEventRecord(e0, nullptr);
                launch();
                (void)hipEventRecord(e1, nullptr);
                if (hipEventSynchronize(e1) != hipSuccess || hipGetLastError() != hipSuccess)
                    rc = fail("ubench: copy kernel failed");
                float t = 0.0f;
                (void)hipEventElapsedTime(&t, e0, e1);
                if (best == 0.0f || t < best)
                    best = t;
            }
            ms = best;
            *out_units = 2.0*(double)(n*sizeof(float4));
        }
    }
    else
    {
        uint32_t nrec = 1;
        while ((unsigned long long)nrec*2ull*64ull <= bytes && nrec < (1u << 30))
            nrec *= 2u;
        if (steps < 1)
            steps = 64;
        const unsigned grid = (unsigned)prop.multiProcessorCount*16u;       // 4 workgroups x 4 waves per SIMD-quad: 16 waves per CU
        DevBuf<float4> recsDev;         // (a record is four float4)
        DevBuf<float> outDev;
        float4* const recs = recsDev.alloc((size_t)nrec*4) ? nullptr : recsDev.get();
        float* const out = outDev.alloc((size_t)grid*256) ? nullptr : outDev.get();
        if (!recs || !out)
            rc = fail("ubench: allocation failed");
        else
        {
            hipLaunchKernelGGL(k_ub_fill, dim3((unsigned)prop.multiProcessorCount*8u), dim3(256), 0, nullptr, recs, nrec);
            auto launch = [&] {
                if (kind == 1) hipLaunchKernelGGL((k_ub_gather<0>), dim3(grid), dim3(256), 0, nullptr, (const float4*)recs, nrec, steps, out);
                else if (kind == 2) hipLaunchKernelGGL((k_ub_gather<1>), dim3(grid), dim3(256), 0, nullptr, (const float4*)recs, nrec, steps, out);
                else hipLaunchKernelGGL((k_ub_gather<2>), dim3(grid), dim3(256), 0, nullptr, (const float4*)recs, nrec, steps, out);
            };
            launch();
            (void)hipEventRecord(e0, nullptr);
            launch();
            (void)hipEventRecord(e1, nullptr);
            if (hipEventSynchronize(e1) != hipSuccess || hipGetLastError() != hipSuccess)
                rc = fail("ubench: gather kernel failed");
            (void)hipEventElapsedTime(&ms, e0, e1);
            *out_units = (double)grid*256.0*(double)steps;
        }
    }
    *out_ms = (double)ms;
    return rc;
}

int tinsel_pack_open(void* blob, size_t size, tinsel_scene_desc* out_scene, tinsel_camera* out_camera, tinsel_options* out_options)
{
    if (!blob || size < sizeof(tinsel_pack_header) || !out_scene)
        return fail("pack_open: bad arguments");
    unsigned char* base = (unsigned char*)blob;
    tinsel_pack_header hdr;
    memcpy(&hdr, base, sizeof(hdr));
    if (memcmp(hdr.magic, TINSEL_PACK_MAGIC, 8) != 0 || hdr.version != 1)
        return fail("pack_open: not a TINPACK1 blob");
    if (hdr.total_bytes > size)
        return fail("pack_open: truncated blob");
    if (hdr.probe_width < 0 || hdr.probe_height < 0)
        return fail("pack_open: negative probe size");

    // written so that nothing can wrap: bytes <= total first, then off <= total - bytes
    auto in_range = [&](uint64_t off, uint64_t bytes) { return off >= sizeof(hdr) && bytes <= hdr.total_bytes && off <= hdr.total_bytes - bytes; };

    if (!in_range(hdr.off_primitives, (uint64_t)hdr.num_primitives*sizeof(tinsel_primitive)) ||
        !in_range(hdr.off_bvh_nodes, (uint64_t)hdr.num_bvh_nodes*sizeof(tinsel_bvh_node)))
        return fail("pack_open: section out of range");

    tinsel_primitive* prims = (tinsel_primitive*)(base + hdr.off_primitives);
    for (uint32_t i = 0; i < hdr.num_primitives; ++i)
    {
        tinsel_primitive& p = prims[i];
        if (p.type != TINSEL_GEOM_MESH)
            continue;
        tinsel_mesh_geometry& g = p.geo.mesh;
        if (g.num_vertices < 0 || g.num_indices < 0 || g.num_nodes < 0)
            return fail("pack_open: negative mesh counts");
        // offsets -> pointers, exactly once (a resolved pointer is far above total_bytes)
        const uint64_t offs[5] = { (uint64_t)(uintptr_t)g.positions, (uint64_t)(uintptr_t)g.normals, (uint64_t)(uintptr_t)g.indices,
                                   (uint64_t)(uintptr_t)g.nodes, (uint64_t)(uintptr_t)g.cdf };
        const uint64_t sizes[5] = { (uint64_t)g.num_vertices*12, (uint64_t)g.num_vertices*12, (uint64_t)g.num_indices*4,
                                    (uint64_t)g.num_nodes*32, (uint64_t)(g.num_indices/3)*4 };
        for (int k = 0; k < 5; ++k)
            if (!in_range(offs[k], sizes[k]))
                return fail("pack_open: mesh section out of range (or pack already opened)");
        g.positions = (const tinsel_vec3*)(base + offs[0]);
        g.normals = (const tinsel_vec3*)(base + offs[1]);
        g.indices = (const int32_t*)(base + offs[2]);
        g.nodes = (const tinsel_bvh_node*)(base + offs[3]);
        g.cdf = (const float*)(base + offs[4]);
    }

    memset(out_scene, 0, sizeof(*out_scene));
    out_scene->primitives = prims;
    out_scene->num_primitives = (int32_t)hdr.num_primitives;
    out_scene->bvh_nodes = (const tinsel_bvh_node*)(base + hdr.off_bvh_nodes);
    out_scene->num_bvh_nodes = (int32_t)hdr.num_bvh_nodes;
    out_scene->sky_horizon = hdr.sky_horizon;
    out_scene->sky_zenith = hdr.sky_zenith;
    if (hdr.off_probe_data)
    {
        const uint64_t n = (uint64_t)hdr.probe_width*hdr.probe_height;
        if (!in_range(hdr.off_probe_data, n*16) || !in_range(hdr.off_probe_pdf_x, n*4) || !in_range(hdr.off_probe_cdf_x, n*4) ||
            !in_range(hdr.off_probe_pdf_y, (uint64_t)hdr.probe_height*4) || !in_range(hdr.off_probe_cdf_y, (uint64_t)hdr.probe_height*4))
            return fail("pack_open: probe section out of range");
        out_scene->probe_valid = 1;
        out_scene->probe_width = hdr.probe_width;
        out_scene->probe_height = hdr.probe_height;
        out_scene->probe_data = (const tinsel_vec4*)(base + hdr.off_probe_data);
        out_scene->probe_pdf_x = (const float*)(base + hdr.off_probe_pdf_x);
        out_scene->probe_cdf_x = (const float*)(base + hdr.off_probe_cdf_x);
        out_scene->probe_pdf_y = (const float*)(base + hdr.off_probe_pdf_y);
        out_scene->probe_cdf_y = (const float*)(base + hdr.off_probe_cdf_y);
    }
    if (out_camera)
        *out_camera = hdr.camera;
    if (out_options)
        *out_options = hdr.options;
    return 0;
}

} // extern "C"

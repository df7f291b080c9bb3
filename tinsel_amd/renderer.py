"""Host-side mirror of the reference's renderer interface over the C-ABI.

Reference interface (src/render.h:66-79):

    struct Renderer { virtual void Init(int w, int h); virtual void Render(const Camera&, const Options&, Color* out); };
    Renderer* CreateGpuRenderer(const Scene* s);

Here: `create_gpu_renderer(scene) -> HipRenderer` with `.init(w, h)` and
`.render(camera, options, output=None, passes=1)`; same argument meaning, same
framebuffer semantics (output == running sum of (rgb*w, w) since init), same
"Init before Render, options.width/height must match Init" contract.  Errors
raise `TinselHipError` carrying tinsel_hip_last_error().

The compute lives entirely in libtinsel_hip.so (hand-written HIP for gfx950).
There is no CPU fallback: without the library or without a GPU these calls raise.
"""
import ctypes as C
import os

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TINSEL_HIP_LIB", os.path.join(_HERE, "libtinsel_hip.so"))     # env: A/B builds only

_lib = None
# The tuning renderers are created with when the caller passes none: None = the library's defaults (tinsel_hip_create).  A plain module
# attribute of THIS binding (tests set it through `use_tuning` to push whole suites through another code path) -- the library itself reads
# no environment variable and has no process-wide state.
DEFAULT_TUNING = None


class TinselHipError(RuntimeError):
    pass


def load_library():
    """dlopen libtinsel_hip.so (once).  torch, when importable, is imported first so that both
    share one HIP runtime (same SONAME libamdhip64.so.7) and torch device pointers are valid here."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise TinselHipError(
            "%s is missing: build it with `python -m tinsel_amd.build` (hipcc, gfx950). "
            "There is no CPU fallback." % LIB_PATH)
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is plumbing, not a requirement of the ABI
        pass
    L = C.CDLL(LIB_PATH)
    vp, ci, cf = C.c_void_p, C.c_int, C.c_float
    L.tinsel_hip_create.restype = vp
    L.tinsel_hip_create.argtypes = [C.POINTER(abi.SceneDesc), ci]
    if hasattr(L, "tinsel_hip_create_tuned"):         # absent from libraries built before round 6 (TINSEL_HIP_LIB: an A/B against an older build)
        L.tinsel_hip_tuning_init.restype = None
        L.tinsel_hip_tuning_init.argtypes = [C.POINTER(abi.Tuning)]
        L.tinsel_hip_create_tuned.restype = vp
        L.tinsel_hip_create_tuned.argtypes = [C.POINTER(abi.SceneDesc), ci, C.POINTER(abi.Tuning)]
        L.tinsel_hip_set_tuning.argtypes = [vp, C.POINTER(abi.Tuning)]
        L.tinsel_hip_get_tuning.argtypes = [vp, C.POINTER(abi.Tuning)]
        L.tinsel_hip_group_create_tuned.restype = vp
        L.tinsel_hip_group_create_tuned.argtypes = [C.POINTER(abi.SceneDesc), ci, ci, C.POINTER(abi.Tuning)]
        L.tinsel_hip_comm_unique_id.argtypes = [vp, ci]
        L.tinsel_hip_comm_init.argtypes = [vp, vp, ci, ci]
        L.tinsel_hip_comm_size.argtypes = [vp]
        L.tinsel_hip_comm_reduce_accum.argtypes = [vp, vp, ci, vp]
    L.tinsel_hip_destroy.restype = None
    L.tinsel_hip_destroy.argtypes = [vp]
    L.tinsel_hip_init.argtypes = [vp, ci, ci]
    L.tinsel_hip_init_external.argtypes = [vp, ci, ci, vp]
    L.tinsel_hip_render.argtypes = [vp, C.POINTER(abi.Camera), C.POINTER(abi.Options), vp, ci]
    L.tinsel_hip_render_async.argtypes = [vp, C.POINTER(abi.Camera), C.POINTER(abi.Options), ci, vp]
    L.tinsel_hip_accum_device_ptr.restype = vp
    L.tinsel_hip_accum_device_ptr.argtypes = [vp]
    L.tinsel_hip_read_accum.argtypes = [vp, vp]
    L.tinsel_hip_set_shard.argtypes = [vp, ci, ci, ci]
    L.tinsel_hip_set_pipeline.argtypes = [vp, ci]
    L.tinsel_hip_set_pass_index.argtypes = [vp, C.c_uint32]
    L.tinsel_hip_get_pass_index.restype = C.c_uint32
    L.tinsel_hip_get_pass_index.argtypes = [vp]
    L.tinsel_hip_stats.restype = None
    L.tinsel_hip_stats.argtypes = [vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), C.POINTER(C.c_double)]
    L.tinsel_hip_reset_stats.restype = None
    L.tinsel_hip_reset_stats.argtypes = [vp]
    L.tinsel_hip_stats_detail.argtypes = [vp, vp]
    L.tinsel_hip_set_detail_counters.argtypes = [vp, ci]
    L.tinsel_hip_render_cost.argtypes = [vp, C.POINTER(abi.Camera), C.POINTER(abi.Options), C.c_uint32, ci, vp]
    L.tinsel_hip_trace_rays.argtypes = [vp, ci, C.c_longlong, vp, vp]
    L.tinsel_hip_trace_rays_device.argtypes = [vp, ci, C.c_longlong, vp, vp, vp]
    L.tinsel_hip_trace_camera.argtypes = [vp, C.POINTER(abi.Camera), ci, ci, cf, vp]
    if hasattr(L, "tinsel_hip_trace_radiance"):        # absent from older builds loaded through TINSEL_HIP_LIB for an A/B
        L.tinsel_hip_trace_radiance.argtypes = [vp, C.c_longlong, vp, ci, vp]
        L.tinsel_hip_trace_radiance_device.argtypes = [vp, C.c_longlong, vp, ci, vp, vp]
    if hasattr(L, "tinsel_hip_gather_radiance"):
        L.tinsel_hip_gather_radiance.argtypes = [vp, ci, C.c_longlong, vp, ci, ci, vp, vp]
        L.tinsel_hip_gather_radiance_device.argtypes = [vp, ci, C.c_longlong, vp, ci, ci, vp, vp, vp]
    if hasattr(L, "tinsel_hip_gather_sh"):
        L.tinsel_hip_gather_sh.argtypes = [vp, ci, ci, C.c_longlong, vp, ci, ci, vp, vp]
        L.tinsel_hip_gather_sh_device.argtypes = [vp, ci, ci, C.c_longlong, vp, ci, ci, vp, vp, vp]
    if hasattr(L, "tinsel_hip_render_features"):       # absent from older builds loaded through TINSEL_HIP_LIB for an A/B
        L.tinsel_hip_render_features.argtypes = [vp, C.POINTER(abi.Camera), C.POINTER(abi.Options), C.c_uint32, ci, C.c_uint, vp]
        L.tinsel_hip_render_features_device.argtypes = [vp, C.POINTER(abi.Camera), C.POINTER(abi.Options), C.c_uint32, ci, C.c_uint, vp, vp]
    if hasattr(L, "tinsel_hip_render_id_mattes"):      # absent from older builds loaded through TINSEL_HIP_LIB for an A/B
        L.tinsel_hip_render_id_mattes.argtypes = [vp, C.POINTER(abi.Camera), C.POINTER(abi.Options), C.c_uint32, ci, ci, vp, vp]
        L.tinsel_hip_render_id_mattes_device.argtypes = [vp, C.POINTER(abi.Camera), C.POINTER(abi.Options), C.c_uint32, ci, ci, vp, vp, vp]
    if hasattr(L, "tinsel_hip_render_light_groups"):   # absent from older builds loaded through TINSEL_HIP_LIB for an A/B
        L.tinsel_hip_render_light_groups.argtypes = [vp, C.POINTER(abi.Camera), C.POINTER(abi.Options), C.c_uint32, ci, ci, vp, ci, vp]
        L.tinsel_hip_render_light_groups_device.argtypes = [vp, C.POINTER(abi.Camera), C.POINTER(abi.Options), C.c_uint32, ci, ci, vp, ci, vp, vp]
    if hasattr(L, "tinsel_hip_render_views"):          # absent from older builds loaded through TINSEL_HIP_LIB for an A/B
        L.tinsel_hip_render_views.argtypes = [vp, C.POINTER(abi.Camera), ci, C.POINTER(abi.Options), C.c_uint32, ci, C.c_uint, vp]
        L.tinsel_hip_render_views_device.argtypes = [vp, C.POINTER(abi.Camera), ci, C.POINTER(abi.Options), C.c_uint32, ci, C.c_uint, vp, vp]
        L.tinsel_hip_plan_views.argtypes = [C.c_ulonglong, ci, ci, ci, ci, C.POINTER(C.c_int)]
    if hasattr(L, "tinsel_hip_render_depth_planes"):   # absent from older builds loaded through TINSEL_HIP_LIB for an A/B
        L.tinsel_hip_render_depth_planes.argtypes = abi.RENDER_DEPTH_PLANES_ARGTYPES
        L.tinsel_hip_render_depth_planes_device.argtypes = abi.RENDER_DEPTH_PLANES_DEVICE_ARGTYPES
    if hasattr(L, "tinsel_hip_render_sample_map"):     # absent from older builds loaded through TINSEL_HIP_LIB for an A/B
        L.tinsel_hip_render_sample_map.argtypes = abi.RENDER_SAMPLE_MAP_ARGTYPES
        L.tinsel_hip_render_sample_map_device.argtypes = abi.RENDER_SAMPLE_MAP_DEVICE_ARGTYPES
        L.tinsel_hip_plan_sample_map.argtypes = abi.PLAN_SAMPLE_MAP_ARGTYPES
    if hasattr(L, "tinsel_hip_denoise"):               # absent from older builds loaded through TINSEL_HIP_LIB for an A/B
        L.tinsel_hip_denoise_params_init.restype = None
        L.tinsel_hip_denoise_params_init.argtypes = [C.POINTER(abi.DenoiseParams)]
        L.tinsel_hip_denoise.argtypes = [vp, vp, vp, C.c_uint, ci, ci, C.POINTER(abi.DenoiseParams), vp]
        L.tinsel_hip_denoise_device.argtypes = [vp, vp, vp, C.c_uint, ci, ci, C.POINTER(abi.DenoiseParams), vp, vp]
        L.tinsel_hip_present_image_device.argtypes = [vp, vp, C.POINTER(abi.Options), ci, C.c_float, vp]
    L.tinsel_hip_kernel_times.argtypes = [vp, C.POINTER(abi.KernelTime), ci]
    L.tinsel_hip_enable_kernel_timing.argtypes = [vp, ci]
    L.tinsel_hip_set_batch_paths.argtypes = [vp, C.c_ulonglong]
    L.tinsel_hip_read_batch_radiance.restype = C.c_longlong
    L.tinsel_hip_read_batch_radiance.argtypes = [vp, vp, C.c_ulonglong]
    L.tinsel_hip_leaf.argtypes = [vp, ci, ci, ci, vp, ci, vp, vp, ci, C.POINTER(abi.Camera), ci, ci]
    L.tinsel_hip_write_accum.argtypes = [vp, vp, C.c_uint32]
    L.tinsel_hip_reserve.argtypes = [vp, ci, ci]
    L.tinsel_hip_set_russian_roulette.argtypes = [vp, ci]
    L.tinsel_hip_set_mesh_bvh.argtypes = [vp, ci, C.POINTER(C.c_double)]
    L.tinsel_hip_present.argtypes = [vp, C.POINTER(abi.Options), ci, C.c_float, vp]
    L.tinsel_hip_present_async.argtypes = [vp, C.POINTER(abi.Options), ci, C.c_float, vp]
    L.tinsel_hip_present_device_ptr.restype = vp
    L.tinsel_hip_present_device_ptr.argtypes = [vp]
    L.tinsel_image_quantize_rgb8.argtypes = [vp, ci, ci, vp]
    L.tinsel_hip_stack_entries.argtypes = [vp]
    if hasattr(L, "tinsel_hip_mesh_tree"):             # absent from older builds loaded through TINSEL_HIP_LIB for an A/B
        L.tinsel_hip_mesh_tree.argtypes = [vp, ci, vp, ci, C.POINTER(C.c_int)]
    L.tinsel_hip_nee_per_path.argtypes = [vp]
    L.tinsel_hip_walked_prims.argtypes = [vp]
    if hasattr(L, "tinsel_hip_walk_tops"):             # absent from older builds loaded through TINSEL_HIP_LIB for an A/B
        L.tinsel_hip_walk_tops.argtypes = [vp, C.POINTER(C.c_int), ci]
    if hasattr(L, "tinsel_hip_bounce_plan"):          # absent from older builds loaded through TINSEL_HIP_LIB for an A/B
        L.tinsel_hip_bounce_plan.argtypes = [vp, C.POINTER(C.c_uint32)]
        L.tinsel_hip_scene_features.restype = C.c_uint
        L.tinsel_hip_scene_features.argtypes = [C.POINTER(abi.SceneDesc)]
    if hasattr(L, "tinsel_hip_scene_slim"):           # absent from older builds loaded through TINSEL_HIP_LIB for an A/B
        L.tinsel_hip_scene_slim.argtypes = [C.POINTER(abi.SceneDesc)]
    if hasattr(L, "tinsel_hip_scene_plane_pairs"):    # absent from older builds loaded through TINSEL_HIP_LIB for an A/B
        L.tinsel_hip_scene_plane_pairs.argtypes = [C.POINTER(abi.SceneDesc), C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int)]
        L.tinsel_hip_plane_table.argtypes = [vp, C.POINTER(C.c_int)]
    if hasattr(L, "tinsel_hip_bake_source"):          # absent from older builds loaded through TINSEL_HIP_LIB for an A/B
        L.tinsel_hip_bake_source.restype = C.c_longlong
        L.tinsel_hip_bake_source.argtypes = [vp, C.c_char_p, C.c_ulonglong, C.c_char_p, C.POINTER(C.c_int)]
        L.tinsel_hip_bake_source_desc.restype = C.c_longlong
        L.tinsel_hip_bake_source_desc.argtypes = [C.POINTER(abi.SceneDesc), C.POINTER(abi.Tuning), C.c_char_p, C.c_ulonglong, C.c_char_p, C.POINTER(C.c_int)]
        L.tinsel_hip_install_baked.argtypes = [vp, C.c_char_p, C.c_ulonglong, C.c_char_p, ci]
        L.tinsel_hip_bake_status.argtypes = [vp, C.POINTER(C.c_uint32), C.c_char_p]
        L.tinsel_hip_set_bounce_bake.argtypes = [vp, ci]
        L.tinsel_hip_get_bounce_bake.argtypes = [vp]
    if hasattr(L, "tinsel_hip_queue_counts"):        # absent from older builds loaded through TINSEL_HIP_LIB for an A/B
        L.tinsel_hip_queue_counts.argtypes = [vp, C.POINTER(C.c_uint32), C.c_int]
    L.tinsel_hip_set_lookahead.argtypes = [vp, ci]
    L.tinsel_hip_refit_mesh.argtypes = [vp, ci, vp, ci, vp]
    if hasattr(L, "tinsel_hip_rebuild_scene"):         # absent from older builds loaded through TINSEL_HIP_LIB for an A/B
        L.tinsel_hip_set_primitive_transform.argtypes = [vp, ci, C.POINTER(abi.Transform), C.POINTER(abi.Transform)]
        L.tinsel_hip_rebuild_scene.argtypes = [vp, ci, vp, ci, C.POINTER(C.c_double)]
    L.tinsel_hip_set_probe_sampling.argtypes = [vp, ci]
    L.tinsel_hip_set_arithmetic.argtypes = [vp, ci]
    L.tinsel_hip_get_arithmetic.argtypes = [vp]
    L.tinsel_hip_group_create.restype = vp
    L.tinsel_hip_group_create.argtypes = [C.POINTER(abi.SceneDesc), ci, ci]
    L.tinsel_hip_group_destroy.restype = None
    L.tinsel_hip_group_destroy.argtypes = [vp]
    L.tinsel_hip_group_init.argtypes = [vp, ci, ci]
    L.tinsel_hip_group_render.argtypes = [vp, C.POINTER(abi.Camera), C.POINTER(abi.Options), vp, ci]
    L.tinsel_hip_group_present.argtypes = [vp, C.POINTER(abi.Options), ci, C.c_float, vp]
    L.tinsel_hip_group_size.argtypes = [vp]
    L.tinsel_hip_group_member.restype = vp
    L.tinsel_hip_group_member.argtypes = [vp, ci]
    L.tinsel_hip_group_set_lookahead.argtypes = [vp, ci]
    L.tinsel_hip_ubench.argtypes = [ci, ci, C.c_ulonglong, ci, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.tinsel_hip_selftest_arith.argtypes = [ci, ci, ci, C.POINTER(C.c_ulonglong), C.POINTER(C.c_uint)]
    if hasattr(L, "tinsel_hip_selftest_sort"):          # (absent from libraries built before round 5: TINSEL_HIP_LIB)
        L.tinsel_hip_selftest_sort.argtypes = [ci, vp, C.c_ulonglong, ci, ci]
        L.tinsel_hip_selftest_scan.argtypes = [ci, vp, vp, C.c_ulonglong]
    if hasattr(L, "tinsel_hip_selftest_accumulate"):    # absent from older builds loaded through TINSEL_HIP_LIB for an A/B
        L.tinsel_hip_selftest_accumulate.argtypes = abi.SELFTEST_ACCUMULATE_ARGTYPES
        L.tinsel_hip_accumulate_support.argtypes = [ci, C.c_float, C.c_float, C.c_float, C.POINTER(C.c_float)]
    L.tinsel_hip_plan_regions.argtypes = [C.c_ulonglong, ci, ci, ci, C.POINTER(C.c_uint)]
    L.tinsel_hip_last_error.restype = C.c_char_p
    L.tinsel_pack_open.argtypes = [vp, C.c_size_t, C.POINTER(abi.SceneDesc), C.POINTER(abi.Camera), C.POINTER(abi.Options)]
    _lib = L
    return L


EXPORTED_SYMBOLS = [
    "tinsel_hip_bake_source", "tinsel_hip_bake_source_desc", "tinsel_hip_install_baked", "tinsel_hip_bake_status", "tinsel_hip_set_bounce_bake", "tinsel_hip_get_bounce_bake",
    "tinsel_hip_bounce_plan", "tinsel_hip_scene_features", "tinsel_hip_scene_slim", "tinsel_hip_scene_plane_pairs", "tinsel_hip_plane_table", "tinsel_hip_create", "tinsel_hip_destroy", "tinsel_hip_init", "tinsel_hip_init_external", "tinsel_hip_render",
    "tinsel_hip_render_async", "tinsel_hip_accum_device_ptr", "tinsel_hip_read_accum", "tinsel_hip_set_shard",
    "tinsel_hip_set_pipeline", "tinsel_hip_set_pass_index", "tinsel_hip_get_pass_index", "tinsel_hip_stats",
    "tinsel_hip_reset_stats", "tinsel_hip_stats_detail", "tinsel_hip_set_detail_counters", "tinsel_hip_render_cost", "tinsel_hip_kernel_times", "tinsel_hip_kernel_time_bytes",
    "tinsel_hip_enable_kernel_timing", "tinsel_hip_set_batch_paths", "tinsel_hip_stack_entries", "tinsel_hip_mesh_tree",
    "tinsel_hip_nee_per_path", "tinsel_hip_last_error", "tinsel_pack_open", "tinsel_hip_read_batch_radiance", "tinsel_hip_leaf",
    "tinsel_hip_write_accum", "tinsel_hip_reserve", "tinsel_hip_set_russian_roulette", "tinsel_hip_set_mesh_bvh", "tinsel_hip_present", "tinsel_hip_present_async", "tinsel_hip_present_device_ptr", "tinsel_image_quantize_rgb8",
    "tinsel_hip_walked_prims", "tinsel_hip_walk_tops", "tinsel_hip_queue_counts", "tinsel_hip_set_lookahead", "tinsel_hip_set_arithmetic", "tinsel_hip_get_arithmetic", "tinsel_hip_refit_mesh", "tinsel_hip_set_probe_sampling",
    "tinsel_hip_set_primitive_transform", "tinsel_hip_rebuild_scene",
    "tinsel_hip_group_create", "tinsel_hip_group_destroy", "tinsel_hip_group_init", "tinsel_hip_group_render", "tinsel_hip_group_present",
    "tinsel_hip_group_size", "tinsel_hip_group_member", "tinsel_hip_group_set_lookahead", "tinsel_hip_ubench",
    "tinsel_hip_selftest_arith", "tinsel_hip_selftest_sort", "tinsel_hip_selftest_scan", "tinsel_hip_selftest_accumulate", "tinsel_hip_accumulate_support", "tinsel_hip_plan_regions",
    "tinsel_hip_tuning_init", "tinsel_hip_create_tuned", "tinsel_hip_set_tuning", "tinsel_hip_get_tuning", "tinsel_hip_group_create_tuned",
    "tinsel_hip_comm_unique_id", "tinsel_hip_comm_init", "tinsel_hip_comm_size", "tinsel_hip_comm_reduce_accum",
    "tinsel_hip_trace_rays", "tinsel_hip_trace_rays_device", "tinsel_hip_trace_camera",
    "tinsel_hip_trace_radiance", "tinsel_hip_trace_radiance_device",
    "tinsel_hip_gather_radiance", "tinsel_hip_gather_radiance_device",
    "tinsel_hip_gather_sh", "tinsel_hip_gather_sh_device",
    "tinsel_hip_render_features", "tinsel_hip_render_features_device",
    "tinsel_hip_render_id_mattes", "tinsel_hip_render_id_mattes_device",
    "tinsel_hip_render_light_groups", "tinsel_hip_render_light_groups_device",
    "tinsel_hip_render_views", "tinsel_hip_render_views_device", "tinsel_hip_plan_views",
    "tinsel_hip_render_sample_map", "tinsel_hip_render_sample_map_device", "tinsel_hip_plan_sample_map",
    "tinsel_hip_render_depth_planes", "tinsel_hip_render_depth_planes_device",
    "tinsel_hip_denoise_params_init", "tinsel_hip_denoise", "tinsel_hip_denoise_device", "tinsel_hip_present_image_device",
]


def rank_id_lists(ids, weights):
    """The ranking of tinsel_hip_render_id_mattes on ids / weights [K, H, W]: per pixel weight descending, ties by ascending id as int32,
    empty slots (abi.ID_EMPTY, weight 0) last.  Returns new arrays."""
    ids, weights = np.asarray(ids, np.int32), np.asarray(weights, np.float32)
    empty = ids == abi.ID_EMPTY
    # np.lexsort: the last key is the primary one
    order = np.lexsort((ids, -weights.astype(np.float64), empty), axis=0)
    return np.take_along_axis(ids, order, 0), np.take_along_axis(weights, order, 0)


def matte(result, ids):
    """The coverage of the primitives `ids` (an id or several; abi.ID_MISS is the background) from what HipRenderer.id_mattes returned:
    float32 [H, W], the sum of the weights of the slots that hold one of the ids divided by the total, 0 where the total is 0 -- the plane a
    compositor multiplies by, anti-aliased, motion-blurred and filtered as the beauty is."""
    wanted = np.isin(np.asarray(result["ids"]), np.atleast_1d(np.asarray(ids, np.int64)))
    wanted &= np.asarray(result["ids"]) != abi.ID_EMPTY
    total = np.asarray(result["total"], np.float32)
    s = np.where(wanted, np.asarray(result["weights"], np.float32), np.float32(0)).sum(axis=0, dtype=np.float32)
    out = np.zeros(total.shape, np.float32)
    np.divide(s, total, out=out, where=total != 0)
    return out


def merge_id_mattes(results, slots):
    """The ranks' partial lists (HipRenderer.id_mattes under set_shard, in rank order) as one list of `slots` slots per pixel: the weights
    of equal ids are summed in rank order (float32), the combined list is ranked by the library's rule, what does not fit in `slots` is
    added to the residual, and the ranks' residuals and totals are summed.  Returns the dict id_mattes returns."""
    results = list(results)
    slots = int(slots)
    if not results or not 1 <= slots:
        raise ValueError("merge_id_mattes: at least one result and one slot")
    H, W = np.asarray(results[0]["total"]).shape
    cap = sum(np.asarray(r["ids"]).shape[0] for r in results)
    ids = np.full((cap, H, W), abi.ID_EMPTY, np.int32)
    weights = np.zeros((cap, H, W), np.float32)
    residual, total = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
    for r in results:
        rid, rw = np.asarray(r["ids"], np.int32), np.asarray(r["weights"], np.float32)
        for k in range(rid.shape[0]):
            c, w = rid[k], rw[k]
            todo = c != abi.ID_EMPTY
            held = (ids == c[None]) & todo[None]
            weights = np.where(held, weights + w[None], weights)
            todo &= ~held.any(axis=0)
            first = np.argmax(ids == abi.ID_EMPTY, axis=0)              # (cap slots: an empty one is always left for a new id)
            jj, ii = np.nonzero(todo)
            ids[first[jj, ii], jj, ii] = c[jj, ii]
            weights[first[jj, ii], jj, ii] = w[jj, ii]
        residual = residual + np.asarray(r["residual"], np.float32)
        total = total + np.asarray(r["total"], np.float32)
    ids, weights = rank_id_lists(ids, weights)
    for k in range(slots, cap):
        residual = residual + weights[k]
    if cap < slots:
        ids = np.concatenate([ids, np.full((slots - cap, H, W), abi.ID_EMPTY, np.int32)])
        weights = np.concatenate([weights, np.zeros((slots - cap, H, W), np.float32)])
    return {"ids": np.ascontiguousarray(ids[:slots]), "weights": np.ascontiguousarray(weights[:slots]), "residual": residual, "total": total}


def rng_state(seed, skip=0):
    """The two words (rng1, rng2 of abi.PathStart) of the reference's Random(seed) after `skip` calls of Rand(): what a radiance query's
    record carries for a path whose generator has made `skip` draws before PathTrace is entered (a camera path: 3 -- x, y, t).
    Vectorised over numpy uint32 (any integer is taken modulo 2^32); returns two uint32 arrays of seed's shape."""
    shape = np.shape(seed)
    s1 = np.asarray(seed).astype(np.uint32).reshape(-1) + np.uint32(315645664)
    s2 = s1 ^ np.uint32(0x13AB45FE)
    for _ in range(int(skip)):
        s1 = (s2 ^ ((s1 << np.uint32(5)) | (s1 >> np.uint32(27)))) ^ (s1*s2)
        s2 = s1 ^ ((s2 << np.uint32(12)) | (s2 >> np.uint32(20)))
    return s1.reshape(shape), s2.reshape(shape)


RAY_EPSILON = 1e-4         # the reference's kRayEpsilon (render.cpp:11): how far a path's next origin is moved off the surface it left


def camera_rays(camera, width, height):
    """CameraSampler::GenerateRay(i, j) of every pixel of a width x height frame (util.h:45-79; the raster position is the pixel's integer
    corner, as trace_camera / first_hit shoot it), restated in float64: (origin [3], unit directions [H, W, 3]).  For placing points on what
    first_hit saw -- the device's own rays are float32, so origin + direction*t lies on the surface to rounding, not to the bit."""
    jj, ii = np.mgrid[0:int(height), 0:int(width)].astype(np.float64)
    f = np.tan(np.float64(camera.fov)*0.5)
    v = np.stack([f*(float(width)/float(height))*(2.0*ii/width - 1.0), f*(1.0 - 2.0*jj/height), -np.ones_like(ii)], axis=-1)
    q = np.array([camera.rotation.x, camera.rotation.y, camera.rotation.z], np.float64)
    w = np.float64(camera.rotation.w)
    t = 2.0*np.cross(q, v)
    d = v + w*t + np.cross(q, t)
    origin = np.array([camera.position.x, camera.position.y, camera.position.z], np.float64)
    return origin, d/np.linalg.norm(d, axis=-1, keepdims=True)


GATHER_MODES = {"cosine": abi.GATHER_COSINE, "sphere": abi.GATHER_SPHERE}


def gather_points(positions, normals, samples, time=1.0, base_seed=0, seeds=None):
    """The point array of a gather query (abi.GATHER_POINT_DTYPE, one record per row of `positions`): positions [n, 3] (the origins as
    given: offset them off the surface first), normals [n, 3] (unit length), `time` a scalar or [n], and the seeds -- by default
    seed_k = base_seed + k*samples modulo 2^32, so that the points' streams (seed_k + s, s < samples) do not meet; `seeds` [n] overrides."""
    positions = np.asarray(positions, np.float32).reshape(-1, 3)
    n = positions.shape[0]
    pts = np.zeros(n, abi.GATHER_POINT_DTYPE)
    pts["px"], pts["py"], pts["pz"] = positions[:, 0], positions[:, 1], positions[:, 2]
    normals = np.asarray(normals, np.float32).reshape(n, 3)
    pts["nx"], pts["ny"], pts["nz"] = normals[:, 0], normals[:, 1], normals[:, 2]
    pts["time"] = np.asarray(time, np.float32)
    if seeds is None:
        seeds = (int(base_seed) + np.arange(n, dtype=np.uint64)*np.uint64(int(samples))) & np.uint64(0xffffffff)
    pts["seed"] = np.asarray(seeds).astype(np.uint32)
    return pts


def sh_basis(directions, order=2):
    """The real orthonormal spherical harmonics of bands 0 .. order (graphics convention) at unit directions [..., 3] -> [..., (order + 1)^2],
    in float32 and in the operation order include/tinsel_hip.h states: the mirror of what tinsel_hip_gather_sh multiplies a path's radiance by."""
    order = int(order)
    if not 0 <= order <= abi.GATHER_SH_MAX_ORDER:
        raise ValueError("sh_basis: order is 0, 1 or 2")
    d = np.asarray(directions, np.float32)
    if d.ndim < 1 or d.shape[-1] != 3:
        raise ValueError("sh_basis: directions [..., 3] are expected")
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    f = np.float32
    Y = [np.full(x.shape, f(0.28209479), np.float32)]
    if order >= 1:
        Y += [f(0.48860251)*y, f(0.48860251)*z, f(0.48860251)*x]
    if order >= 2:
        Y += [(f(1.0925484)*x)*y, (f(1.0925484)*y)*z, f(0.31539157)*((f(3.0)*z)*z - f(1.0)), (f(1.0925484)*x)*z, f(0.54627422)*(x*x - y*y)]
    out = np.stack(Y, axis=-1)
    assert out.dtype == np.float32
    return out


SH_COSINE_LOBE = (np.pi, 2.0*np.pi/3.0, np.pi/4.0)        # the clamped cosine's zonal factors A_l of bands 0, 1, 2


def sh_irradiance(coeffs, normals):
    """Irradiance from SH radiance coefficients, in float64: E(n) = sum_i A_l(i) c_i Y_i(n), A = pi, 2 pi/3, pi/4 for bands 0, 1, 2.
    `coeffs` [n, C, 3] (or [C, 3]: one probe) are the coefficients of the incident radiance, already scaled -- 4 pi * the means of a
    sphere-mode gather_sh; `normals` [n, 3] unit vectors, one per probe, or [m, 3] against one probe.  Returns [n, 3] (or [m, 3])."""
    c = np.asarray(coeffs, np.float64)
    nrm = np.asarray(normals, np.float64).reshape(-1, 3)
    if c.ndim == 2:
        c = c[None]
    if c.ndim != 3 or c.shape[1] not in (1, 4, 9) or c.shape[2] != 3 or (c.shape[0] != 1 and c.shape[0] != nrm.shape[0]):
        raise ValueError("sh_irradiance: coeffs [n, C, 3] with C = 1, 4 or 9 and normals [n, 3] (or [m, 3] against one probe) are expected")
    order = {1: 0, 4: 1, 9: 2}[c.shape[1]]
    x, y, z = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    Y = [np.full(x.shape, 0.5*np.sqrt(1.0/np.pi))]
    if order >= 1:
        k = np.sqrt(3.0/(4.0*np.pi))
        Y += [k*y, k*z, k*x]
    if order >= 2:
        k = 0.5*np.sqrt(15.0/np.pi)
        Y += [k*x*y, k*y*z, 0.25*np.sqrt(5.0/np.pi)*(3.0*z*z - 1.0), k*x*z, 0.5*k*(x*x - y*y)]
    band = np.array([SH_COSINE_LOBE[l] for l in (0, 1, 1, 1, 2, 2, 2, 2, 2)][:c.shape[1]])
    return np.einsum("ni,nic->nc", np.stack(Y, axis=-1)*band, np.broadcast_to(c, (nrm.shape[0],) + c.shape[1:]))


def feature_mask(which):
    """The TINSEL_FEATURE_* bits of an iterable of plane names (abi.FEATURE_NAMES) -- or of an int, taken as the mask itself -- and the
    names of its planes in the order the library writes them (ascending bit order)"""
    if isinstance(which, (int, np.integer)):
        mask = int(which)
    else:
        names = [which] if isinstance(which, str) else list(which)
        for n in names:
            if n not in abi.FEATURE_NAMES:
                raise ValueError("features: %r is not one of %s" % (n, ", ".join(abi.FEATURE_NAMES)))
        mask = sum(1 << abi.FEATURE_NAMES.index(n) for n in set(names))
    return mask, [n for k, n in enumerate(abi.FEATURE_NAMES) if 0 <= mask <= 7 and mask >> k & 1]


def feature_images(planes):
    """The images a denoiser or a compositor takes, from the raw planes of HipRenderer.features (name -> [H, W, 4]: weighted sum xyz,
    weight sum w), in float64 -- of the planes that are there:
      "albedo" [H, W, 3]          xyz/w
      "normal" [H, W, 3]          xyz/w brought to unit length; 0 where the mean is 0
      "depth" [H, W]              x/z: the mean depth over the samples that hit something
      "depth_variance" [H, W]     y/z - (x/z)^2
      "coverage" [H, W]           z/w: the share of the filter weight that hit something (alpha)
    and 0 wherever the divisor (w, or the depth plane's z) is 0."""
    def ratio(num, den):
        den = np.asarray(den, np.float64)
        ok = den != 0.0
        return np.where(ok, np.asarray(num, np.float64)/np.where(ok, den, 1.0), 0.0)

    out = {}
    if "albedo" in planes:
        a = np.asarray(planes["albedo"], np.float64)
        out["albedo"] = ratio(a[..., :3], a[..., 3:4])
    if "normal" in planes:
        a = np.asarray(planes["normal"], np.float64)
        mean = ratio(a[..., :3], a[..., 3:4])
        out["normal"] = ratio(mean, np.sqrt((mean*mean).sum(axis=-1, keepdims=True)))
    if "depth" in planes:
        a = np.asarray(planes["depth"], np.float64)
        mean = ratio(a[..., 0], a[..., 2])
        out["depth"] = mean
        out["depth_variance"] = np.where(a[..., 2] != 0.0, ratio(a[..., 1], a[..., 2]) - mean*mean, 0.0)
        out["coverage"] = ratio(a[..., 2], a[..., 3])
    return out


def default_light_groups(scene, max_groups=abi.MAX_LIGHT_GROUPS):
    """A grouping for HipRenderer.light_groups: (group_of_primitive int32 [num_primitives], env_group, names).  Every primitive with
    non-zero emission, in index order, gets a group of its own ("prim<i>"); when there are more of them than fit, the rest share the last
    light group; the environment ("env") gets the group after the lights if the scene has a probe or a non-zero sky, else env_group is
    -1.  Primitives that do not emit are in no group (-1)."""
    max_groups = int(max_groups)
    if not 1 <= max_groups <= abi.MAX_LIGHT_GROUPS:
        raise ValueError("default_light_groups: max_groups is 1 .. %d" % abi.MAX_LIGHT_GROUPS)
    d = scene.desc
    prims = C.cast(d.primitives, C.POINTER(abi.Primitive))
    emitters = [i for i in range(d.num_primitives) if any(v != 0.0 for v in prims[i].material.emission)]
    env = bool(d.probe_valid) or any(v != 0.0 for v in tuple(d.sky_horizon) + tuple(d.sky_zenith))
    room = max_groups - (1 if env else 0)
    if emitters and room < 1:
        raise ValueError("default_light_groups: max_groups = %d leaves no group for the lights beside the environment" % max_groups)
    table = np.full(d.num_primitives, -1, np.int32)
    names = []
    for k, i in enumerate(emitters):
        g = min(k, room - 1)
        table[i] = g
        if g == len(names):
            names.append("prim%d" % i)
        elif not names[g].endswith("+"):
            names[g] += "+"
    env_group = -1
    if env:
        env_group = len(names)
        names.append("env")
    return table, env_group, names


def _quat_mul(a, b):
    """Hamilton product of two quaternions (x, y, z, w): the rotation b followed by the rotation a"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw*bx + ax*bw + ay*bz - az*by, aw*by - ax*bz + ay*bw + az*bx, aw*bz + ax*by - ay*bx + az*bw, aw*bw - ax*bx - ay*by - az*bz])


def _quat_rotate(q, v):
    """q*v*q^-1 for a unit quaternion (x, y, z, w)"""
    u, w = np.asarray(q[:3], np.float64), float(q[3])
    v = np.asarray(v, np.float64)
    return v + 2.0*np.cross(u, np.cross(u, v) + w*v)


def orbit_cameras(camera, center, count, axis=(0, 1, 0)):
    """A turntable for HipRenderer.views: `count` copies of `camera` (abi.Camera), copy k rotated by 2*pi*k/count about the line through
    `center` along `axis` -- the position is turned about the centre and the rotation with it, so the camera keeps looking at what it
    looked at; fov and shutter are kept.  Copy 0 is the camera itself, bit for bit.  The arithmetic runs in float64 and is rounded to the
    camera's float32 once."""
    count = int(count)
    if count < 1:
        raise ValueError("orbit_cameras: count must be >= 1")
    n = np.asarray(axis, np.float64).reshape(3)
    if not np.isfinite(n).all() or not np.linalg.norm(n) > 0.0:
        raise ValueError("orbit_cameras: axis must be a finite non-zero vector")
    n = n/np.linalg.norm(n)
    c = np.asarray(center, np.float64).reshape(3)
    p0, q0 = np.array(tuple(camera.position), np.float64), np.array(tuple(camera.rotation), np.float64)
    out = (abi.Camera*count)()
    for k in range(count):
        cam = abi.Camera.from_buffer_copy(bytes(camera))
        if k:
            a = 2.0*np.pi*k/count
            q = np.concatenate([n*np.sin(0.5*a), [np.cos(0.5*a)]])
            p = c + _quat_rotate(q, p0 - c)
            r = _quat_mul(q, q0)
            cam.position = abi.Vec3(*(float(v) for v in p))
            cam.rotation = abi.Vec4(*(float(v) for v in r))
        out[k] = cam
    return out


def cube_cameras(position, shutter=(0.0, 0.0)):
    """The six faces of a cube map around `position` for HipRenderer.views: cameras with a 90-degree field of view (render them at a
    square frame size) looking along +x, -x, +y, -y, +z, -z, in that order.  The convention is the reference's camera (CameraSampler): a
    camera looks along its local -z, its local +y is the top of the image and its local +x the right.  Up, the top of the image, is
    world +y on the four side faces (+x, -x, +z, -z), world +z on the +y face and world -z on the -y face: the -z face is the identity
    rotation, the other sides are it turned about y, and the +y / -y faces are it pitched up / down by 90 degrees about x."""
    s = float(np.sqrt(0.5))
    quats = [(0.0, -s, 0.0, s), (0.0, s, 0.0, s), (s, 0.0, 0.0, s), (-s, 0.0, 0.0, s), (0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0)]
    out = (abi.Camera*6)()
    for k, q in enumerate(quats):
        out[k] = abi.Camera(abi.Vec3(*(float(v) for v in position)), abi.Vec4(*q), float(np.pi/2), float(shutter[0]), float(shutter[1]))
    return out


def plan_views(slot_limit, width, height, passes, num_views):
    """tinsel_hip_plan_views: (views per batch, passes per batch, batches) of a views call under a limit of slot_limit path slots per batch
    (host arithmetic only, no GPU needed)"""
    L = load_library()
    out = (C.c_int*3)()
    _check(L.tinsel_hip_plan_views(int(slot_limit), int(width), int(height), int(passes), int(num_views), out), "tinsel_hip_plan_views")
    return tuple(int(v) for v in out)


def _sample_counts(counts, width, height, who):
    """the map as the C entries read it: a C-contiguous uint16 array [H, W]"""
    counts = np.asarray(counts)
    if counts.dtype != np.uint16 or counts.shape != (int(height), int(width)):
        raise ValueError("%s: counts is a uint16 array [%d, %d]" % (who, int(height), int(width)))
    return np.ascontiguousarray(counts)


def plan_sample_map(slot_limit, width, height, counts):
    """tinsel_hip_plan_sample_map: (levels per batch, batches, total paths, largest count) of a sample-map call with the uint16 map
    `counts` [H, W] under a limit of slot_limit path slots per batch (host arithmetic only, no GPU needed)"""
    L = load_library()
    counts = _sample_counts(counts, width, height, "plan_sample_map")
    out = (C.c_ulonglong*4)()
    _check(L.tinsel_hip_plan_sample_map(int(slot_limit), int(width), int(height), _host_ptr(counts), out), "tinsel_hip_plan_sample_map")
    return tuple(int(v) for v in out)


def crop_sample_map(width, height, x0, y0, x1, y1, passes):
    """A crop for HipRenderer.sample_map: uint16 [height, width], `passes` on the pixels x0 <= i < x1, y0 <= j < y1 (cut to the frame) and
    0 elsewhere.  The call then gives those pixels' samples of a full-frame render of `passes` passes -- and, splatted by the filter, their
    share of the pixels within its reach; a pixel farther out stays exactly zero."""
    passes = int(passes)
    if not 0 <= passes <= abi.SAMPLE_MAP_MAX:
        raise ValueError("crop_sample_map: passes must be in 0 .. %d" % abi.SAMPLE_MAP_MAX)
    counts = np.zeros((int(height), int(width)), np.uint16)
    counts[max(0, int(y0)):max(0, int(y1)), max(0, int(x0)):max(0, int(x1))] = passes
    return counts


def relight(planes, gains):
    """The light mix: sum over g of gains[g]*planes[g] for planes [G, H, W, 4] (HipRenderer.light_groups) -- a gain is a scalar or an RGB
    triple per group -- as an accumulator: float32 [H, W, 4] whose weight channel is plane 0's (every plane carries the beauty's), so the
    result drops into present_image and denoise.  numpy arrays or torch tensors (the result is of the planes' kind); the sum runs in
    float32, groups ascending."""
    G = int(planes.shape[0])
    if planes.ndim != 4 or planes.shape[-1] != 4 or G < 1:
        raise ValueError("relight: planes [G, H, W, 4] are expected")
    g = np.asarray(gains, np.float32)
    if g.shape not in ((G,), (G, 3)):
        raise ValueError("relight: one gain, or one RGB triple, per group is expected: shape (%d,) or (%d, 3)" % (G, G))
    g = np.broadcast_to(g.reshape(G, -1), (G, 3))
    if _is_tensor(planes):
        import torch
        gt = torch.as_tensor(np.ascontiguousarray(g), device=planes.device)
        out = planes[0].clone()
        out[..., :3] = planes[0][..., :3]*gt[0]
        for k in range(1, G):
            out[..., :3] += planes[k][..., :3]*gt[k]
        return out
    planes = np.asarray(planes, np.float32)
    out = planes[0].copy()
    out[..., :3] = planes[0][..., :3]*g[0]
    for k in range(1, G):
        out[..., :3] += planes[k][..., :3]*g[k]
    return out


def depth_contributions(planes):
    """What each depth adds: float32 [n, H, W, 3] from the planes [n, H, W, 4] of HipRenderer.depth_planes.  Entry 0 is plane 0's image --
    colour divided by weight, 0 where the weight is 0 -- and entry k is image k minus image k - 1: for depths 1 .. D direct light (with
    what the camera sees of the emitters), then each further bounce's share.  The shares add up to the deepest plane's image within fp32
    rounding.  With options.clamp = FLT_MAX no share is negative; a FINITE clamp applies to each plane's samples separately and can make a
    share negative.  numpy arrays or torch tensors (the result is of the planes' kind)."""
    if planes.ndim != 4 or planes.shape[-1] != 4 or int(planes.shape[0]) < 1:
        raise ValueError("depth_contributions: planes [n, H, W, 4] are expected")
    if _is_tensor(planes):
        import torch
        w = planes[..., 3:4]
        img = torch.where(w != 0, planes[..., :3]/torch.where(w != 0, w, torch.ones_like(w)), torch.zeros_like(planes[..., :3]))
        out = img.clone()
        out[1:] = img[1:] - img[:-1]
        return out
    planes = np.asarray(planes, np.float32)
    w = planes[..., 3:4]
    img = np.where(w != 0, planes[..., :3]/np.where(w != 0, w, np.float32(1)), np.float32(0)).astype(np.float32)
    out = img.copy()
    out[1:] = img[1:] - img[:-1]
    return out


def denoise_params(**fields):
    """tinsel_hip_denoise_params: the library's defaults (tinsel_hip_denoise_params_init) with `fields` over them -- radius, patch_radius,
    k_color, k_albedo, k_normal, k_depth, demodulate, albedo_floor"""
    p = abi.DenoiseParams()
    load_library().tinsel_hip_denoise_params_init(C.byref(p))
    names = [k for k, _ in abi.DenoiseParams._fields_]
    for k, v in fields.items():
        if k not in names:
            raise TypeError("tinsel_hip_denoise_params has no field %r" % k)
        setattr(p, k, v)
    return p


def _is_tensor(a):
    return a is not None and not isinstance(a, np.ndarray) and hasattr(a, "data_ptr")


def _check(rc, what):
    if rc != 0:
        msg = load_library().tinsel_hip_last_error()
        raise TinselHipError("%s failed: %s" % (what, msg.decode() if msg else "?"))


def _host_ptr(a):
    """The address of a numpy array for the library (the pointer object keeps the array alive).  An empty array's data pointer may be
    null: a one-element stand-in gives the library an address it can check."""
    return (a if a.size else np.zeros(1, a.dtype)).ctypes.data_as(C.c_void_p)


class Scene:
    """A scene as the C-ABI sees it: a `SceneDesc` plus the camera/options the scene file carried.

    Scenes come from scene packs (DESIGN.md "Scene pack"): one relocatable blob written by the
    reference's own loader + Scene::Build (tests/golden/make_golden.py).
    """

    def __init__(self, blob: bytes):
        L = load_library()
        self._buf = C.create_string_buffer(blob, len(blob))     # owned, writable: pack_open relocates in place
        self.desc = abi.SceneDesc()
        self.camera = abi.Camera()
        self.options = abi.Options()
        _check(L.tinsel_pack_open(self._buf, len(blob), C.byref(self.desc), C.byref(self.camera), C.byref(self.options)),
               "tinsel_pack_open")

    @classmethod
    def load_pack(cls, path):
        with open(path, "rb") as fh:
            return cls(fh.read())

    @property
    def num_primitives(self):
        return self.desc.num_primitives

    def bounce_features(self):
        """tinsel_hip_scene_features: the abi.BOUNCE_* bits this scene asks of the fused kernel (no device needed)"""
        return int(load_library().tinsel_hip_scene_features(C.byref(self.desc)))

    def bounce_slim(self):
        """tinsel_hip_scene_slim: do this scene's paths carry the slim state in the fused kernel's compiled instances (no device needed)"""
        return bool(load_library().tinsel_hip_scene_slim(C.byref(self.desc)))

    def plane_pairs(self):
        """tinsel_hip_scene_plane_pairs: ([(a, b), ...], singles) -- the pairing rule on this scene's always-hit planes, as primitive indices,
        and how many of them stay single (no device needed).  Whether a renderer has a plane table and pairs in it is decided at create
        (include/tinsel_hip.h); HipRenderer.plane_table() reports it."""
        n = max(1, self.num_primitives//2)
        out = (C.c_int32*(2*n))()
        singles = C.c_int(0)
        k = load_library().tinsel_hip_scene_plane_pairs(C.byref(self.desc), out, n, C.byref(singles))
        return [(out[2*q], out[2*q + 1]) for q in range(k)], singles.value

    def bake_source(self, tuning=None):
        """tinsel_hip_bake_source_desc: (text, key, bakeable, why) -- the generated header a baked instance of this scene is compiled from, its
        key (the sha256 of the text) and whether a renderer of the scene under `tuning` would be planned with the closed instance, with
        the failing condition where it would not (no device needed)"""
        L = load_library()
        return _bake_source(lambda buf, cap, key, ok: L.tinsel_hip_bake_source_desc(C.byref(self.desc), C.byref(tuning) if tuning is not None else None, buf, cap, key, ok))


def _bake_source(call):
    """the two-call pattern of tinsel_hip_bake_source*: length first, then the text"""
    key = C.create_string_buffer(65)
    ok = C.c_int(0)
    n = call(None, 0, key, C.byref(ok))
    if n < 0:
        raise RuntimeError("tinsel_hip_bake_source: " + load_library().tinsel_hip_last_error().decode())
    why = "" if ok.value else load_library().tinsel_hip_last_error().decode()
    buf = C.create_string_buffer(int(n) + 1)
    call(buf, int(n) + 1, key, C.byref(ok))
    return buf.value.decode(), key.value.decode(), bool(ok.value), why


def _bytes_at(ptr, n):
    return C.string_at(ptr, n) if (ptr and n > 0) else b""


_libc = C.CDLL(None)
_libc.memcmp.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]


def _same_bytes(pa, pb, n):
    """memcmp of two host arrays in place (a frame's mesh arrays are tens of MB: no copies)"""
    if n <= 0 or pa == pb:
        return True
    return bool(pa) and bool(pb) and _libc.memcmp(pa, pb, n) == 0


def _same_nodes(pa, pb, n):
    """two reference-format trees node by node.  Not just a byte compare: a leaf's rightIndex bits are whatever the reference builder's heap
    held (bvh.h:236-237 sets leftIndex and `leaf` only) and may differ from one load of the same file to the next."""
    if n <= 0 or _same_bytes(pa, pb, n*32):
        return True
    a = np.ctypeslib.as_array((C.c_uint32*(n*8)).from_address(pa)).reshape(n, 8)
    b = np.ctypeslib.as_array((C.c_uint32*(n*8)).from_address(pb)).reshape(n, 8)
    if not np.array_equal(a[:, :7], b[:, :7]):                      # bounds (6 floats as bits) + leftIndex
        return False
    leaf_a, leaf_b = a[:, 7] >> 31, b[:, 7] >> 31
    if not np.array_equal(leaf_a, leaf_b):
        return False
    inner = leaf_a == 0
    return bool(np.array_equal(a[inner, 7], b[inner, 7]))


def scene_delta(old: Scene, new: Scene):
    """What turns a renderer created from `old` into one for `new` WITHOUT re-uploading anything: ([(primitive, start, end)], the new scene
    BVH's nodes) when `new` is `old` with other primitive transforms -- the frames of a rigid animation, what the reference's batch mode
    re-loads and re-creates per frame (main.cpp:314-327) -- else None (geometry, materials, lights, sky or probe differ: re-create)."""
    a, b = old.desc, new.desc
    if a.num_primitives != b.num_primitives or bytes(a.sky_horizon) != bytes(b.sky_horizon) or bytes(a.sky_zenith) != bytes(b.sky_zenith):
        return None
    if (a.probe_valid, a.probe_width, a.probe_height) != (b.probe_valid, b.probe_width, b.probe_height):
        return None
    if a.probe_valid and not _same_bytes(a.probe_data, b.probe_data, a.probe_width*a.probe_height*16):
        return None
    P = a.num_primitives
    pa, pb = (abi.Primitive*P).from_address(a.primitives), (abi.Primitive*P).from_address(b.primitives)
    moves = []
    for i in range(P):
        x, y = pa[i], pb[i]
        mx, my = bytes(x.material), bytes(y.material)
        # (the material's parameters: bytes [0, 84) and [112, 128); between them padding and the bump-map texture -- a host pointer and sizes
        # the integrator never reads: bump mapping is dead code in the reference)
        if x.type != y.type or x.light_samples != y.light_samples or mx[:84] != my[:84] or mx[112:] != my[112:]:
            return None
        if x.type == abi.GEOM_SPHERE and x.geo.sphere.radius != y.geo.sphere.radius:
            return None
        if x.type == abi.GEOM_PLANE and bytes(x.geo.plane) != bytes(y.geo.plane):
            return None
        if x.type == abi.GEOM_MESH:
            g, h = x.geo.mesh, y.geo.mesh
            if (g.num_vertices, g.num_indices, g.num_nodes, g.area) != (h.num_vertices, h.num_indices, h.num_nodes, h.area):
                return None
            for f, n in (("positions", g.num_vertices*12), ("normals", g.num_vertices*12), ("indices", g.num_indices*4), ("cdf", (g.num_indices//3)*4)):
                if not _same_bytes(getattr(g, f), getattr(h, f), n):
                    return None
            if not _same_nodes(g.nodes, h.nodes, g.num_nodes):
                return None
        if bytes(x.start_transform) != bytes(y.start_transform) or bytes(x.end_transform) != bytes(y.end_transform):
            moves.append((i, abi.Transform.from_buffer_copy(bytes(y.start_transform)), abi.Transform.from_buffer_copy(bytes(y.end_transform))))
    nodes = (abi.BVHNode*b.num_bvh_nodes).from_buffer_copy(_bytes_at(b.bvh_nodes, b.num_bvh_nodes*C.sizeof(abi.BVHNode)))
    return moves, nodes


class HipRenderer:
    """`Renderer` (render.h:66-73) implemented by the gfx950 streaming path tracer."""

    def __init__(self, scene: Scene, device: int = 0, tuning: "abi.Tuning | None" = None):
        L = load_library()
        self._L = L
        tuning = tuning if tuning is not None else DEFAULT_TUNING
        if tuning is None:
            self._h = L.tinsel_hip_create(C.byref(scene.desc), device)
        else:
            self._h = L.tinsel_hip_create_tuned(C.byref(scene.desc), device, C.byref(tuning))
        if not self._h:
            msg = L.tinsel_hip_last_error()
            raise TinselHipError("tinsel_hip_create failed: %s" % (msg.decode() if msg else "?"))
        if tuning is not None:
            self._apply_bake_mode(tuning)
        self.device = device
        self.num_primitives = int(scene.desc.num_primitives)     # (light_groups: the table the library reads has one entry each)
        self.width = self.height = 0
        self._accum_tensor = None

    # bake mode 1 ("at the next reserve() or first fused render, whatever the size"): what a render checks before it starts.  The mode and
    # the key of the last attempt that did not install are kept on this side, so that modes -1 and 0 cost a render one comparison
    _bake_mode = -1
    _bake_failed_key = None

    def _bake_before_render(self):
        if self._bake_mode == 1:
            self.bake()

    # -- Renderer interface ------------------------------------------------
    def init(self, width, height, accum_tensor=None):
        """Renderer::Init: (re)allocate + zero the accumulator.  `accum_tensor`: optional torch
        float32 device tensor [H,W,4] to use as the accumulator (for an RCCL reduce)."""
        if accum_tensor is not None:
            assert tuple(accum_tensor.shape) == (height, width, 4) and accum_tensor.is_contiguous()
            self._accum_tensor = accum_tensor
            _check(self._L.tinsel_hip_init_external(self._h, width, height, accum_tensor.data_ptr()), "tinsel_hip_init_external")
        else:
            self._accum_tensor = None
            _check(self._L.tinsel_hip_init(self._h, width, height), "tinsel_hip_init")
        self.width, self.height = width, height

    def render(self, camera, options, output=None, passes=1, readback=True):
        """Renderer::Render: add `passes` samples per pixel; returns the running sum [H,W,4] (rgb*w, w)."""
        if output is None and readback:
            output = np.empty((options.height, options.width, 4), np.float32)
        ptr = output.ctypes.data_as(C.c_void_p) if (readback and output is not None) else None
        self._bake_before_render()
        _check(self._L.tinsel_hip_render(self._h, C.byref(camera), C.byref(options), ptr, passes), "tinsel_hip_render")
        return output

    Init = init
    Render = render

    # -- beyond the reference interface -------------------------------------
    def render_async(self, camera, options, passes=1, stream=None):
        self._bake_before_render()
        _check(self._L.tinsel_hip_render_async(self._h, C.byref(camera), C.byref(options), passes, stream), "tinsel_hip_render_async")

    def read_accum(self):
        out = np.empty((self.height, self.width, 4), np.float32)
        _check(self._L.tinsel_hip_read_accum(self._h, out.ctypes.data_as(C.c_void_p)), "tinsel_hip_read_accum")
        return out

    def set_mesh_bvh(self, mode):
        """abi.BVH_REFERENCE (the reference's host-built trees, parity path) or abi.BVH_LBVH (rebuild large meshes on
        the device); returns the device build time in ms."""
        ms = C.c_double(0.0)
        _check(self._L.tinsel_hip_set_mesh_bvh(self._h, int(mode), C.byref(ms)), "tinsel_hip_set_mesh_bvh")
        return ms.value

    def write_accum(self, accum, next_pass_index):
        """Restores a saved accumulator [H,W,4] and the index of the next pass (resume a progressive render)."""
        accum = np.ascontiguousarray(accum, np.float32)
        assert accum.shape == (self.height, self.width, 4)
        _check(self._L.tinsel_hip_write_accum(self._h, accum.ctypes.data_as(C.c_void_p), int(next_pass_index)), "tinsel_hip_write_accum")

    def present(self, options, nlm_width=0, nlm_falloff=200.0, readback=True):
        """The display stage of the reference's frame loop (main.cpp:258-282) on the device accumulator:
        normalise by the filter weight, ToneMap, LinearToSrgb, optional NonLocalMeansFilter.
        Returns the float image [H,W,4] main.cpp presents / hands to WritePng."""
        out = np.empty((self.height, self.width, 4), np.float32) if readback else None
        ptr = out.ctypes.data_as(C.c_void_p) if readback else None
        _check(self._L.tinsel_hip_present(self._h, C.byref(options), int(nlm_width), float(nlm_falloff), ptr), "tinsel_hip_present")
        return out

    @property
    def accum_tensor(self):
        return self._accum_tensor

    def accum_device_ptr(self):
        return self._L.tinsel_hip_accum_device_ptr(self._h)

    def set_shard(self, rank, world, tile=32):
        _check(self._L.tinsel_hip_set_shard(self._h, rank, world, tile), "tinsel_hip_set_shard")

    def set_pipeline(self, pipeline):
        _check(self._L.tinsel_hip_set_pipeline(self._h, pipeline), "tinsel_hip_set_pipeline")

    # -- the process-per-GPU arm of the one collective (tinsel_hip_comm_*): the library's own ncclReduce, the id carried by the host language
    @staticmethod
    def comm_unique_id():
        """bytes of an RCCL unique id (rank 0 makes it, the host language hands it to the other ranks)"""
        buf = (C.c_ubyte*abi.COMM_ID_BYTES)()
        _check(load_library().tinsel_hip_comm_unique_id(buf, abi.COMM_ID_BYTES), "tinsel_hip_comm_unique_id")
        return bytes(buf)

    def comm_init(self, id_bytes, rank, world):
        """collective: every rank calls it with rank 0's id"""
        buf = (C.c_ubyte*abi.COMM_ID_BYTES).from_buffer_copy(bytes(id_bytes))
        _check(self._L.tinsel_hip_comm_init(self._h, buf, int(rank), int(world)), "tinsel_hip_comm_init")

    def comm_size(self):
        """ranks of this renderer's RCCL communicator as RCCL counts them (ncclCommCount); 0: none"""
        return int(self._L.tinsel_hip_comm_size(self._h)) if hasattr(self._L, "tinsel_hip_comm_size") else 0

    def comm_reduce_accum(self, out_ptr, root=0, stream=None):
        """sum of every rank's accumulator into device memory `out_ptr` (W*H*4 floats) on `root`; waits for `stream`"""
        _check(self._L.tinsel_hip_comm_reduce_accum(self._h, out_ptr, int(root), stream), "tinsel_hip_comm_reduce_accum")

    def set_tuning(self, tuning=None, **fields):
        """tinsel_hip_set_tuning: the per-render fields of an abi.Tuning (or of the tuning in force with `fields` replaced); the create-time
        fields (abi.Tuning.CREATE_FIELDS) belong to create_gpu_renderer(scene, device, tuning)."""
        t = (tuning if tuning is not None else self.get_tuning()).replace(**fields)
        # (the binding's own fields alone: no field of the C struct changes, so the path buffers tinsel_hip_set_tuning frees are kept)
        if not (tuning is None and fields and set(fields) <= set(abi.Tuning.BINDING_FIELDS)):
            _check(self._L.tinsel_hip_set_tuning(self._h, C.byref(t)), "tinsel_hip_set_tuning")
        self._apply_bake_mode(t)

    def _apply_bake_mode(self, tuning):
        """abi.Tuning's `bounce_bake` is carried beside the C struct (abi.Tuning.BINDING_FIELDS): handed over through its own setter"""
        if hasattr(self._L, "tinsel_hip_set_bounce_bake"):
            _check(self._L.tinsel_hip_set_bounce_bake(self._h, int(tuning.bounce_bake)), "tinsel_hip_set_bounce_bake")
            self._bake_mode = int(tuning.bounce_bake)

    def plane_table(self):
        """tinsel_hip_plane_table: (opposing pairs, single planes) of the flat scan's plane table in force"""
        out = (C.c_int*2)()
        _check(self._L.tinsel_hip_plane_table(self._h, out), "tinsel_hip_plane_table")
        return out[0], out[1]

    def get_tuning(self):
        t = abi.Tuning()
        _check(self._L.tinsel_hip_get_tuning(self._h, C.byref(t)), "tinsel_hip_get_tuning")
        if hasattr(self._L, "tinsel_hip_get_bounce_bake"):
            t.bounce_bake = int(self._L.tinsel_hip_get_bounce_bake(self._h))
        return t

    def set_arithmetic(self, mode):
        """abi.ARITH_EXACT (default: bit-identical to the CPU reference) or abi.ARITH_FAST (FMA / rcp / hardware transcendentals:
        the reference's own -ffast-math trade, inside the 1e-3 L2 bar but not bit-reproducible)."""
        _check(self._L.tinsel_hip_set_arithmetic(self._h, int(mode)), "tinsel_hip_set_arithmetic")

    def refit_mesh(self, primitive, positions, normals=None):
        """New vertex positions [V,3] (and optionally normals) for `primitive`'s mesh, same topology: boxes refitted on the device."""
        positions = np.ascontiguousarray(positions, np.float32)
        nptr = None
        if normals is not None:
            normals = np.ascontiguousarray(normals, np.float32)
            nptr = normals.ctypes.data_as(C.c_void_p)
        _check(self._L.tinsel_hip_refit_mesh(self._h, int(primitive), positions.ctypes.data_as(C.c_void_p), int(positions.shape[0]), nptr),
               "tinsel_hip_refit_mesh")

    def set_primitive_transform(self, index, start, end=None):
        """Primitive `index` moves: new start / end transforms (abi.Transform; end defaults to start).  Follow with rebuild_scene()."""
        end = start if end is None else end
        _check(self._L.tinsel_hip_set_primitive_transform(self._h, int(index), C.byref(start), C.byref(end)), "tinsel_hip_set_primitive_transform")

    def rebuild_scene(self, nodes=None):
        """The scene-level BVH from the primitives as they are now: from `nodes` (a ctypes array of abi.BVHNode, e.g. the reference's own
        Scene::Build -- bit-identical to a fresh renderer) or, without, built on the device.  Returns the device build time in ms."""
        ms = C.c_double(0.0)
        if nodes is None:
            rc = self._L.tinsel_hip_rebuild_scene(self._h, abi.SCENE_BVH_DEVICE, None, 0, C.byref(ms))
        else:
            rc = self._L.tinsel_hip_rebuild_scene(self._h, abi.SCENE_BVH_NODES, C.cast(nodes, C.c_void_p), len(nodes), C.byref(ms))
        _check(rc, "tinsel_hip_rebuild_scene")
        return ms.value

    def update_scene(self, old: Scene, new: Scene):
        """The next frame of an animation on THIS renderer: when `new` is `old` (the scene this renderer holds) with other primitive transforms,
        the moved primitives' records are rewritten in place and the scene level is rebuilt from `new`'s own nodes (the reference's
        Scene::Build for that frame) -- bit-identical to a renderer created from `new`, nothing re-uploaded.  False (and nothing changed)
        when the frames differ in more than that: the caller re-creates, as the reference always does (main.cpp:318-327)."""
        d = scene_delta(old, new)
        if d is None:
            return False
        moves, nodes = d
        for i, s, e in moves:
            self.set_primitive_transform(i, s, e)
        self.rebuild_scene(nodes)
        return True

    def set_probe_sampling(self, mode):
        """abi.PROBE_CDF (the reference's binary searches: sample-identical) or abi.PROBE_ALIAS (O(1) alias table: same distribution)."""
        _check(self._L.tinsel_hip_set_probe_sampling(self._h, int(mode)), "tinsel_hip_set_probe_sampling")

    def set_lookahead(self, on):
        """Trace the next call's passes while this call's image is copied out (tinsel_hip_set_lookahead); images unchanged.
        abi.LOOKAHEAD_PIN_OUTPUT also page-locks the output array in place (it must then outlive the renderer / the next init)."""
        _check(self._L.tinsel_hip_set_lookahead(self._h, int(on)), "tinsel_hip_set_lookahead")

    def set_russian_roulette(self, start_bounce):
        """0 (default) = none, as the reference; b > 0 = roulette from bounce b on (unbiased, not sample-identical)."""
        _check(self._L.tinsel_hip_set_russian_roulette(self._h, int(start_bounce)), "tinsel_hip_set_russian_roulette")

    def reserve(self, passes, max_depth):
        """Pre-allocates the path buffers for renders of up to `passes` passes at `max_depth`.  Where the plan picks the fused kernel's closed
        instance, this is also where its baked instance is compiled (or found in the cache) and installed: always with the bake mode
        (abi.Tuning's bounce_bake, tinsel_hip_set_bounce_bake) 1, by default (-1) for reservations of abi.BAKE_AUTO_MIN_PATHS path slots or
        more, never with 0.  With mode 1 the first render after a change of the scene level bakes too (render, render_async)."""
        _check(self._L.tinsel_hip_reserve(self._h, int(passes), int(max_depth)), "tinsel_hip_reserve")
        want = self.get_tuning().bounce_bake if hasattr(self._L, "tinsel_hip_bake_source") else 0
        if want > 0 or (want < 0 and int(passes)*self.width*self.height >= abi.BAKE_AUTO_MIN_PATHS):
            self.bake()

    def bake_source(self):
        """tinsel_hip_bake_source: (text, key, bakeable, why) for the scene level in force (Scene.bake_source is the description's twin)"""
        return _bake_source(lambda buf, cap, key, ok: self._L.tinsel_hip_bake_source(self._h, buf, cap, key, ok))

    def bake(self):
        """Compiles (tinsel_amd.build.bake: a child process, cached by key) and installs the baked instance of the scene level in force, where
        the plan would pick the closed instance and none is installed for this key yet.  Never an error: without a compiler, or where the
        compile fails or its code object is refused (build.bake), the library's own instance keeps running and bake_status() says so; a key
        that did not install is not tried again until the scene level, and with it the key, changes.  Returns bake_status()."""
        from . import build as hb
        st = self.bake_status()
        if st["state"] in (abi.BAKE_NONE, abi.BAKE_STALE, abi.BAKE_NO_COMPILER):
            text, key, ok, _ = self.bake_source()
            if key == self._bake_failed_key:
                return st
            image, how = hb.bake(text, key) if ok else (None, None)
            self._bake_failed_key = key if (ok and image is None) else None
            if image is not None:
                _check(self._L.tinsel_hip_install_baked(self._h, image, len(image), key.encode(), abi.BAKE_FROM_CACHE if how == "cache" else abi.BAKE_COMPILED),
                       "tinsel_hip_install_baked")
            elif ok:
                _check(self._L.tinsel_hip_install_baked(self._h, None, 0, None, abi.BAKE_NO_COMPILER), "tinsel_hip_install_baked")
            st = self.bake_status()
        return st

    def bake_status(self):
        """tinsel_hip_bake_status: {"state": abi.BAKE_*, "key": the installed module's key or "", "launches": launches it has served}"""
        out = (C.c_uint32*3)()
        key = C.create_string_buffer(65)
        _check(self._L.tinsel_hip_bake_status(self._h, out, key), "tinsel_hip_bake_status")
        return {"state": int(out[0]), "key": key.value.decode(), "launches": int(out[1]) | (int(out[2]) << 32)}

    def get_pass_index(self):
        """Index of the next pass (its seed is the (index+1)-th output of Random(1).Rand())."""
        return int(self._L.tinsel_hip_get_pass_index(self._h))

    def set_pass_index(self, i):
        _check(self._L.tinsel_hip_set_pass_index(self._h, i), "tinsel_hip_set_pass_index")

    def set_batch_paths(self, n):
        _check(self._L.tinsel_hip_set_batch_paths(self._h, n), "tinsel_hip_set_batch_paths")

    def set_detail_counters(self, on):
        _check(self._L.tinsel_hip_set_detail_counters(self._h, int(on)), "tinsel_hip_set_detail_counters")

    def render_cost(self, camera, options, pass_begin=0, passes=1):
        """Per-pixel traversal cost of path tracing passes [pass_begin, pass_begin + passes): an (H, W, 4) uint32 array of
        {rays, internal BVH node visits, triangle tests, primitive tests} summed over the passes, as the reference algorithm
        counts them (the quantities of stats_detail, on the scene BVH walk).  Pixels another shard owns are 0.  Leaves the
        accumulator, pass index, statistics and tuning as they were (tinsel_hip_render_cost)."""
        out = np.zeros((options.height, options.width, 4), np.uint32)
        _check(self._L.tinsel_hip_render_cost(self._h, C.byref(camera), C.byref(options), int(pass_begin), int(passes),
                                              out.ctypes.data_as(C.c_void_p)), "tinsel_hip_render_cost")
        return out

    def features(self, camera, options, pass_begin=0, passes=1, which=abi.FEATURE_NAMES, out=None):
        """Feature buffers (tinsel_hip_render_features*): the first-hit albedo, shading normal and depth of the beauty's own camera samples
        of passes [pass_begin, pass_begin + passes), accumulated with options.filter exactly as the beauty is -- a dict name -> [H, W, 4]
        float32 of the planes `which` names ("albedo", "normal", "depth"): xyz the weighted sum, w the weight sum (feature_images turns them
        into albedo, unit normal, depth, depth variance and coverage).  `out`: a contiguous float32 torch tensor [planes, H, W, 4] on this
        renderer's device takes the device entry on torch's current stream, not waited for, and the dict holds views of it; a numpy array
        of that shape is filled by the host entry.  Needs init() at the options' frame size; leaves the accumulator, pass index, pass
        seeds, statistics and tuning as they were."""
        mask, names = feature_mask(which)
        H, W = int(options.height), int(options.width)
        shape = (max(len(names), 1), H, W, 4)
        if out is not None and not isinstance(out, np.ndarray) and hasattr(out, "data_ptr"):
            import torch
            if out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous() or not out.is_cuda:
                raise ValueError("features: a contiguous float32 tensor %s on the GPU is expected" % (shape,))
            if out.device.index != self.device:
                raise ValueError("features: the tensor is on %s, the renderer on device %d" % (out.device, self.device))
            _check(self._L.tinsel_hip_render_features_device(self._h, C.byref(camera), C.byref(options), int(pass_begin), int(passes), mask,
                                                             out.data_ptr(), torch.cuda.current_stream(out.device).cuda_stream),
                   "tinsel_hip_render_features_device")
        else:
            if out is None:
                out = np.zeros(shape, np.float32)
            elif out.dtype != np.float32 or out.shape != shape or not out.flags.c_contiguous:
                raise ValueError("features: a C-contiguous float32 array %s is expected" % (shape,))
            _check(self._L.tinsel_hip_render_features(self._h, C.byref(camera), C.byref(options), int(pass_begin), int(passes), mask,
                                                      out.ctypes.data_as(C.c_void_p)), "tinsel_hip_render_features")
        return {n: out[k] for k, n in enumerate(names)}

    def light_groups(self, camera, options, pass_begin, passes, groups, env_group=None, out=None):
        """Light groups (tinsel_hip_render_light_groups*): the beauty of passes [pass_begin, pass_begin + passes) split by which emitter
        produced it, in one trace -- float32 [G, H, W, 4], plane g the accumulator a render would give with every emitter outside group g
        black (bit for bit; options.clamp applies per plane).  `groups`: int [num_primitives], the group of each primitive's emission, -1
        for none (default_light_groups makes one); env_group: the sky's / probe's group (None or -1: none).  G is the highest group
        named + 1.  `out`: a contiguous float32 torch tensor [G, H, W, 4] on this renderer's device takes the device entry on torch's
        current stream, not waited for; a numpy array of that shape is filled by the host entry.  Needs init() at the options' frame size;
        leaves the accumulator, pass index, pass seeds and statistics as they were.  relight() mixes the planes."""
        table = np.ascontiguousarray(np.asarray(groups).reshape(-1), np.int32)
        env = -1 if env_group is None else int(env_group)
        if out is not None:
            G = int(out.shape[0])
        else:
            G = max(int(table.max()) if table.size else -1, env) + 1
        if table.size != self.num_primitives:
            raise ValueError("light_groups: groups has %d entries, the scene %d primitives" % (table.size, self.num_primitives))
        H, W = int(options.height), int(options.width)
        shape = (max(G, 1), H, W, 4)
        if _is_tensor(out):
            import torch
            if out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous() or not out.is_cuda:
                raise ValueError("light_groups: a contiguous float32 tensor %s on the GPU is expected" % (shape,))
            if out.device.index != self.device:
                raise ValueError("light_groups: the tensor is on %s, the renderer on device %d" % (out.device, self.device))
            _check(self._L.tinsel_hip_render_light_groups_device(self._h, C.byref(camera), C.byref(options), int(pass_begin), int(passes), G,
                                                                 _host_ptr(table), env, out.data_ptr(), torch.cuda.current_stream(out.device).cuda_stream),
                   "tinsel_hip_render_light_groups_device")
        else:
            if out is None:
                out = np.zeros(shape, np.float32)
            elif out.dtype != np.float32 or out.shape != shape or not out.flags.c_contiguous:
                raise ValueError("light_groups: a C-contiguous float32 array %s is expected" % (shape,))
            _check(self._L.tinsel_hip_render_light_groups(self._h, C.byref(camera), C.byref(options), int(pass_begin), int(passes), G,
                                                          _host_ptr(table), env, out.ctypes.data_as(C.c_void_p)), "tinsel_hip_render_light_groups")
        return out

    def depth_planes(self, camera, options, pass_begin, passes, depths=None, out=None, add=False, singly=False):
        """Depth planes (tinsel_hip_render_depth_planes*): the beauty of passes [pass_begin, pass_begin + passes) at several path depths in
        one trace -- float32 [n, H, W, 4], plane k the accumulator render() gives from zero with options.max_depth = depths[k] (bit for bit;
        options.clamp applies per plane, the Russian-roulette setting applies).  `depths`: strictly ascending ints in 1 .. 64, at most 16;
        None: 1 .. options.max_depth.  options.max_depth itself is not read by the call.  add: the passes are added to what `out` holds
        instead of starting every plane from zero; singly: one accumulate launch per plane instead of one per batch (the same bits).
        `out`: a contiguous float32 torch tensor [n, H, W, 4] on this renderer's device takes the device entry on torch's current stream,
        not waited for; a numpy array of that shape is filled by the host entry.  Needs init() at the options' frame size; leaves the
        accumulator, pass index, pass seeds and statistics as they were.  depth_contributions() turns the planes into per-bounce shares."""
        if depths is None:
            if int(options.max_depth) > abi.MAX_DEPTH_PLANES:
                raise ValueError("depth_planes: options.max_depth = %d is more than %d planes: name the depths" % (int(options.max_depth), abi.MAX_DEPTH_PLANES))
            depths = range(1, int(options.max_depth) + 1)
        table = np.ascontiguousarray(np.asarray(list(depths)).reshape(-1), np.int32)
        n = int(table.size)
        flags = (abi.DEPTH_PLANES_ADD if add else 0) | (abi.DEPTH_PLANES_ACCUMULATE_SINGLY if singly else 0)
        H, W = int(options.height), int(options.width)
        shape = (max(n, 1), H, W, 4)
        if _is_tensor(out):
            import torch
            if out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous() or not out.is_cuda:
                raise ValueError("depth_planes: a contiguous float32 tensor %s on the GPU is expected" % (shape,))
            if out.device.index != self.device:
                raise ValueError("depth_planes: the tensor is on %s, the renderer on device %d" % (out.device, self.device))
            _check(self._L.tinsel_hip_render_depth_planes_device(self._h, C.byref(camera), C.byref(options), int(pass_begin), int(passes), n,
                                                                 _host_ptr(table), flags, out.data_ptr(), torch.cuda.current_stream(out.device).cuda_stream),
                   "tinsel_hip_render_depth_planes_device")
        else:
            if out is None:
                if add:
                    raise ValueError("depth_planes: add=True needs the planes to add to (out)")
                out = np.zeros(shape, np.float32)
            elif out.dtype != np.float32 or out.shape != shape or not out.flags.c_contiguous:
                raise ValueError("depth_planes: a C-contiguous float32 array %s is expected" % (shape,))
            _check(self._L.tinsel_hip_render_depth_planes(self._h, C.byref(camera), C.byref(options), int(pass_begin), int(passes), n,
                                                          _host_ptr(table), flags, out.ctypes.data_as(C.c_void_p)), "tinsel_hip_render_depth_planes")
        return out

    def views(self, cameras, options, pass_begin=0, passes=1, out=None, add=False, singly=False):
        """View batches (tinsel_hip_render_views*): the frames of many cameras on the resident scene in one call -- float32 [V, H, W, 4],
        plane v the accumulator render() gives for cameras[v] from a zeroed accumulator at pass index pass_begin after `passes` passes, bit
        for bit.  `cameras`: a sequence of abi.Camera or a ctypes array of them (orbit_cameras and cube_cameras make one).  add: the passes
        are added to what `out` holds instead of starting every plane from zero; singly: one accumulate launch per view instead of one per
        batch of views (the same bits).  `out`: a contiguous float32 torch tensor [V, H, W, 4] on this renderer's device takes the device
        entry on torch's current stream, not waited for; a numpy array of that shape is filled by the host entry.  Needs init() at the
        options' frame size; leaves the accumulator, pass index, pass seeds, statistics and tuning as they were."""
        if not isinstance(cameras, C.Array):
            cameras = list(cameras)
            cameras = (abi.Camera*len(cameras))(*cameras)
        V = len(cameras)
        cams = C.cast(cameras, C.POINTER(abi.Camera))
        flags = (abi.VIEWS_ADD if add else 0) | (abi.VIEWS_ACCUMULATE_SINGLY if singly else 0)
        H, W = int(options.height), int(options.width)
        shape = (V, H, W, 4)
        if _is_tensor(out):
            import torch
            if out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous() or not out.is_cuda:
                raise ValueError("views: a contiguous float32 tensor %s on the GPU is expected" % (shape,))
            if out.device.index != self.device:
                raise ValueError("views: the tensor is on %s, the renderer on device %d" % (out.device, self.device))
            _check(self._L.tinsel_hip_render_views_device(self._h, cams, V, C.byref(options), int(pass_begin), int(passes), flags,
                                                          out.data_ptr(), torch.cuda.current_stream(out.device).cuda_stream),
                   "tinsel_hip_render_views_device")
        else:
            if out is None:
                if add:
                    raise ValueError("views: add=True needs the planes to add to (out)")
                out = np.zeros(shape, np.float32)
            elif out.dtype != np.float32 or out.shape != shape or not out.flags.c_contiguous:
                raise ValueError("views: a C-contiguous float32 array %s is expected" % (shape,))
            _check(self._L.tinsel_hip_render_views(self._h, cams, V, C.byref(options), int(pass_begin), int(passes), flags,
                                                   out.ctypes.data_as(C.c_void_p)), "tinsel_hip_render_views")
        return out

    def sample_map(self, camera, options, counts, pass_begin=0, out=None, add=False):
        """Sample maps (tinsel_hip_render_sample_map*): a per-pixel pass count in one call -- float32 [H, W, 4], AddSample of the samples of
        levels 0 .. counts[j, i] - 1 of every pixel, level t the path render() starts for the pixel in pass pass_begin + t; a uniform map n
        is the accumulator of n passes from zero at pass_begin, bit for bit.  `counts`: a numpy uint16 array [H, W] (crop_sample_map makes
        one), read before the call returns.  add: the samples are added to what `out` holds instead of starting from zero.  `out`: a
        contiguous float32 torch tensor [H, W, 4] on this renderer's device takes the device entry on torch's current stream and stays on
        the device; a numpy array of that shape is filled by the host entry.  Needs init() at the options' frame size; leaves the
        accumulator, pass index, pass seeds, statistics and tuning as they were."""
        H, W = int(options.height), int(options.width)
        counts = _sample_counts(counts, W, H, "sample_map")
        flags = abi.SAMPLES_ADD if add else 0
        shape = (H, W, 4)
        if _is_tensor(out):
            import torch
            if out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous() or not out.is_cuda:
                raise ValueError("sample_map: a contiguous float32 tensor %s on the GPU is expected" % (shape,))
            if out.device.index != self.device:
                raise ValueError("sample_map: the tensor is on %s, the renderer on device %d" % (out.device, self.device))
            _check(self._L.tinsel_hip_render_sample_map_device(self._h, C.byref(camera), C.byref(options), int(pass_begin), _host_ptr(counts), flags,
                                                               out.data_ptr(), torch.cuda.current_stream(out.device).cuda_stream),
                   "tinsel_hip_render_sample_map_device")
        else:
            if out is None:
                if add:
                    raise ValueError("sample_map: add=True needs the plane to add to (out)")
                out = np.zeros(shape, np.float32)
            elif out.dtype != np.float32 or out.shape != shape or not out.flags.c_contiguous:
                raise ValueError("sample_map: a C-contiguous float32 array %s is expected" % (shape,))
            _check(self._L.tinsel_hip_render_sample_map(self._h, C.byref(camera), C.byref(options), int(pass_begin), _host_ptr(counts), flags,
                                                        out.ctypes.data_as(C.c_void_p)), "tinsel_hip_render_sample_map")
        return out

    def id_mattes(self, camera, options, pass_begin=0, passes=1, slots=6, out=None):
        """ID mattes (tinsel_hip_render_id_mattes*): per pixel the ranked list of (primitive id, filter-weight sum) pairs of the beauty's own
        camera samples of passes [pass_begin, pass_begin + passes), filtered with options.filter exactly as the beauty is -- a dict
        {"ids": int32 [slots, H, W] (abi.ID_MISS: the path left the scene, abi.ID_EMPTY: an unused slot), "weights": float32 [slots, H, W],
        "residual": [H, W] (what found no slot), "total": [H, W] (the accumulator's w)}, weight descending.  tinsel_amd.matte turns it into
        the coverage of a set of ids.  `out`: a pair of contiguous torch tensors on this renderer's device, int32 [slots, H, W] and float32
        [slots + 2, H, W], takes the device entry on torch's current stream, not waited for, and the dict holds views of them; a pair of
        numpy arrays of those shapes is filled by the host entry.  Needs init() at the options' frame size; leaves the accumulator, pass
        index, pass seeds, statistics and tuning as they were.  Under a shard the result is this rank's partial list (merge_id_mattes)."""
        slots = int(slots)
        H, W = int(options.height), int(options.width)
        ishape, wshape = (max(slots, 0), H, W), (max(slots, 0) + 2, H, W)
        if out is not None and len(out) != 2:
            raise ValueError("id_mattes: out is a pair (ids, weights)")
        if out is not None and hasattr(out[0], "data_ptr") and not isinstance(out[0], np.ndarray):
            import torch
            ids, weights = out
            for t, dtype, shape in ((ids, torch.int32, ishape), (weights, torch.float32, wshape)):
                if not hasattr(t, "data_ptr") or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or not t.is_cuda:
                    raise ValueError("id_mattes: contiguous tensors int32 %s and float32 %s on the GPU are expected" % (ishape, wshape))
                if t.device.index != self.device:
                    raise ValueError("id_mattes: the tensor is on %s, the renderer on device %d" % (t.device, self.device))
            _check(self._L.tinsel_hip_render_id_mattes_device(self._h, C.byref(camera), C.byref(options), int(pass_begin), int(passes), slots,
                                                              ids.data_ptr(), weights.data_ptr(), torch.cuda.current_stream(ids.device).cuda_stream),
                   "tinsel_hip_render_id_mattes_device")
        else:
            if out is None:
                ids, weights = np.zeros(ishape, np.int32), np.zeros(wshape, np.float32)
            else:
                ids, weights = out
                for a, dtype, shape in ((ids, np.int32, ishape), (weights, np.float32, wshape)):
                    if not isinstance(a, np.ndarray) or a.dtype != dtype or a.shape != shape or not a.flags.c_contiguous:
                        raise ValueError("id_mattes: C-contiguous arrays int32 %s and float32 %s are expected" % (ishape, wshape))
            _check(self._L.tinsel_hip_render_id_mattes(self._h, C.byref(camera), C.byref(options), int(pass_begin), int(passes), slots,
                                                       ids.ctypes.data_as(C.c_void_p), weights.ctypes.data_as(C.c_void_p)), "tinsel_hip_render_id_mattes")
        return {"ids": ids, "weights": weights[:slots], "residual": weights[slots], "total": weights[slots + 1]}

    def _image_tensor(self, who, t, shape):
        import torch
        if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous() or not t.is_cuda:
            raise ValueError("%s: a contiguous float32 tensor %s on the GPU is expected" % (who, shape))
        if t.device.index != self.device:
            raise ValueError("%s: the tensor is on %s, the renderer on device %d" % (who, t.device, self.device))
        return t

    def denoise(self, planes=None, params=None, beauty=None, out=None):
        """The feature-guided denoise stage (tinsel_hip_denoise*): a joint non-local-means filter on linear radiance.  `beauty`: an
        accumulator-form image [H, W, 4] (xyz the sum, w the weight), None = this renderer's own accumulator; `planes`: what features()
        returns -- a dict name -> [H, W, 4] -- or None for no guides; `params`: denoise_params(...), None = the defaults.  Returns the
        denoised radiance [H, W, 4] with w = 1, which present_image takes.  numpy arrays go through the host entry and numpy comes back;
        where beauty, a plane or `out` is a torch tensor on this renderer's device everything given must be one, the device entry runs on
        torch's current stream, not waited for, and a tensor comes back (`out` when given).  Leaves the accumulator, pass index, statistics
        and tuning as they were."""
        params = params if params is not None else denoise_params()
        planes = dict(planes) if planes else {}
        mask, names = feature_mask(tuple(planes))
        given = [beauty, out] + [planes[n] for n in names]
        on_device = any(_is_tensor(a) for a in given)
        if beauty is not None:
            H, W = int(beauty.shape[0]), int(beauty.shape[1])
        elif names:
            H, W = int(planes[names[0]].shape[0]), int(planes[names[0]].shape[1])
        else:
            H, W = self.height, self.width
        shape = (H, W, 4)
        if on_device:
            import torch
            if any(a is not None and not _is_tensor(a) for a in given):
                raise ValueError("denoise: beauty, planes and out are either all numpy arrays or all tensors on the GPU")
            dev = next(a for a in given if a is not None).device
            stack = None
            if names:
                for n in names:
                    self._image_tensor("denoise", planes[n], shape)
                # (the planes of one features() tensor are neighbours already: no copy)
                first = planes[names[0]]
                step = H*W*4*4
                if all(planes[n].data_ptr() == first.data_ptr() + k*step for k, n in enumerate(names)):
                    stack = first
                else:
                    stack = torch.stack([planes[n] for n in names])
            if beauty is not None:
                self._image_tensor("denoise", beauty, shape)
            out = self._image_tensor("denoise", out, shape) if out is not None else torch.empty(shape, dtype=torch.float32, device=dev)
            _check(self._L.tinsel_hip_denoise_device(self._h, beauty.data_ptr() if beauty is not None else None,
                                                     stack.data_ptr() if stack is not None else None, mask, W, H, C.byref(params), out.data_ptr(),
                                                     torch.cuda.current_stream(dev).cuda_stream), "tinsel_hip_denoise_device")
            return out
        stack = None
        if names:
            stack = np.ascontiguousarray(np.stack([np.asarray(planes[n], np.float32) for n in names]))
            if stack.shape != (len(names),) + shape:
                raise ValueError("denoise: every plane is an array %s" % (shape,))
        if beauty is not None:
            beauty = np.ascontiguousarray(beauty, np.float32)
            if beauty.shape != shape:
                raise ValueError("denoise: the beauty is an array [H, W, 4]")
        if out is None:
            out = np.empty(shape, np.float32)
        elif out.dtype != np.float32 or out.shape != shape or not out.flags.c_contiguous:
            raise ValueError("denoise: a C-contiguous float32 array %s is expected" % (shape,))
        _check(self._L.tinsel_hip_denoise(self._h, _host_ptr(beauty) if beauty is not None else None, _host_ptr(stack) if stack is not None else None,
                                          mask, W, H, C.byref(params), out.ctypes.data_as(C.c_void_p)), "tinsel_hip_denoise")
        return out

    def present_image(self, image, options, nlm_width=0, nlm_falloff=200.0):
        """The display stage (present) on `image` in place of the accumulator (tinsel_hip_present_image_device): any accumulator-form
        image [H, W, 4] of the init size -- what denoise() returns, a reduced frame.  A torch tensor on this renderer's device is read
        where it is, on torch's current stream, and the presented image comes back as a tensor; a numpy array is uploaded first and
        numpy comes back."""
        shape = (self.height, self.width, 4)
        import torch
        host = not _is_tensor(image)
        if host:
            a = np.ascontiguousarray(image, np.float32)
            if a.shape != shape:
                raise ValueError("present_image: an array %s is expected" % (shape,))
            image = torch.from_numpy(a).to("cuda:%d" % self.device)
        self._image_tensor("present_image", image, shape)
        stream = torch.cuda.current_stream(image.device)
        _check(self._L.tinsel_hip_present_image_device(self._h, image.data_ptr(), C.byref(options), int(nlm_width), float(nlm_falloff), stream.cuda_stream),
               "tinsel_hip_present_image_device")
        ptr = self._L.tinsel_hip_present_device_ptr(self._h)
        out = torch.empty(shape, dtype=torch.float32, device=image.device)
        # (the HIP runtime the library is linked against, found through the library's own handle: device to device, on the same stream)
        copy = self._L.hipMemcpyAsync
        copy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        if copy(out.data_ptr(), ptr, out.numel()*4, 3, stream.cuda_stream) != 0:
            raise TinselHipError("present_image: the copy of the presented image failed")
        if host:
            return out.cpu().numpy()
        return out

    def _records(self, who, arg, width, record=None):
        """The record array of trace_rays / radiance / gather: (n, its address, torch device, stream).  A contiguous (n, width) torch tensor
        on this renderer's device -- float32, or int32 too where the records hold integers (`record` given) -- is for the device entry on
        torch's current stream.  Anything else is for the host entry and the device is None: a numpy array of the dtype abi.<record> or an
        (n, width) array of 32-bit words -- without `record`, whatever converts to (n, width) float32."""
        if not isinstance(arg, np.ndarray) and hasattr(arg, "data_ptr"):
            import torch
            dtypes = (torch.float32, torch.int32) if record else (torch.float32,)
            if arg.dtype not in dtypes or arg.dim() != 2 or arg.shape[1] != width or not arg.is_contiguous() or not arg.is_cuda:
                raise ValueError("%s: a contiguous (n, %d) %s tensor on the GPU is expected" % (who, width, "float32 or int32" if record else "float32"))
            if arg.device.index != self.device:
                raise ValueError("%s: the tensor is on %s, the renderer on device %d" % (who, arg.device, self.device))
            return int(arg.shape[0]), arg.data_ptr(), arg.device, torch.cuda.current_stream(arg.device).cuda_stream
        if record is None:
            words = np.ascontiguousarray(arg, np.float32)
            if words.ndim != 2 or words.shape[1] != width:
                raise ValueError("%s: an (n, %d) float32 array is expected" % (who, width))
        else:
            words = np.asarray(arg)
            if not (words.dtype == np.dtype(getattr(abi, record)) and words.ndim == 1) and \
               not (words.dtype.itemsize == 4 and words.dtype.kind in "fiu" and words.ndim == 2 and words.shape[1] == width):
                raise ValueError("%s: an array of abi.%s or an (n, %d) array of 32-bit words is expected" % (who, record, width))
            words = np.ascontiguousarray(words)
        return words.shape[0], _host_ptr(words), None, None

    def trace_rays(self, rays, mode="closest"):
        """Ray queries on the resident scene (tinsel_hip_trace_rays*): `rays` is an (n, 8) float32 array of
        (origin xyz, time, direction xyz, tmax) -- a numpy array (host entry; returns numpy) or a contiguous torch tensor on this
        renderer's device (device entry on torch's current stream, not waited for; returns a torch tensor).
        mode "closest": a record array of abi.RAY_HIT_DTYPE (t, primitive, nx, ny, nz; a miss: FLT_MAX, -1, 0) -- from torch an
        (n, 8) float32 tensor holding the same 32-byte records; "occluded": uint32 (torch: int32) 1 / 0 for `0 < t < tmax`.
        Leaves the accumulator, pass index, statistics and tuning as they were; needs no init()."""
        modes = {"closest": abi.QUERY_CLOSEST, "occluded": abi.QUERY_OCCLUDED, abi.QUERY_CLOSEST: abi.QUERY_CLOSEST, abi.QUERY_OCCLUDED: abi.QUERY_OCCLUDED}
        if mode not in modes:
            raise ValueError("trace_rays: mode is 'closest' or 'occluded'")
        m = modes[mode]
        n, ptr, device, stream = self._records("trace_rays", rays, 8)
        if device is not None:
            import torch
            out = torch.empty((n, 8), dtype=torch.float32, device=device) if m == abi.QUERY_CLOSEST else \
                torch.empty((n,), dtype=torch.int32, device=device)
            if n:
                _check(self._L.tinsel_hip_trace_rays_device(self._h, m, n, ptr, out.data_ptr(), stream), "tinsel_hip_trace_rays_device")
            return out
        out = np.zeros(n, abi.RAY_HIT_DTYPE) if m == abi.QUERY_CLOSEST else np.zeros(n, np.uint32)
        _check(self._L.tinsel_hip_trace_rays(self._h, m, n, ptr, _host_ptr(out)), "tinsel_hip_trace_rays")
        return out

    def radiance(self, starts, max_depth):
        """Radiance queries on the resident scene (tinsel_hip_trace_radiance*): the reference's PathTrace for paths the caller starts,
        one per record of `starts` -- a numpy array of abi.PATH_START_DTYPE, or an (n, 12) array of 32-bit words holding the same
        48-byte records (origin xyz, time, direction xyz -- unit length, used as given --, a reserved word, rng1, rng2 from rng_state,
        two reserved words): the host entry, returns float32 (n, 4) = radiance rgb + a reserved word, unclamped and unfiltered.  A
        contiguous (n, 12) float32 / int32 torch tensor on this renderer's device goes to the device entry on torch's current stream,
        not waited for, and a float32 (n, 4) tensor comes back.  Uses the scene in force and the roulette, probe-sampling and arithmetic
        settings; leaves the accumulator, pass index and tuning as they were; its rays and samples are counted in stats(); needs no init()."""
        max_depth = int(max_depth)
        n, ptr, device, stream = self._records("radiance", starts, 12, "PATH_START_DTYPE")
        if device is not None:
            import torch
            out = torch.empty((n, 4), dtype=torch.float32, device=device)
            if n:
                _check(self._L.tinsel_hip_trace_radiance_device(self._h, n, ptr, max_depth, out.data_ptr(), stream), "tinsel_hip_trace_radiance_device")
            return out
        out = np.zeros((n, 4), np.float32)
        _check(self._L.tinsel_hip_trace_radiance(self._h, n, ptr, max_depth, _host_ptr(out)), "tinsel_hip_trace_radiance")
        return out

    def gather(self, points, samples, max_depth, mode="cosine", return_starts=False):
        """Gather queries on the resident scene (tinsel_hip_gather_radiance*): `samples` paths from each point, drawn on the device --
        sample s of point k from Random(seed_k + s), two draws, a cosine-weighted direction about the normal (mode "cosine": mean * pi is
        the irradiance) or a uniform one on the sphere ("sphere": the mean incident radiance) -- path-traced as radiance() traces them and
        summed in ascending s: float32 (n, 4) = mean radiance rgb + 0.  `points`: a numpy array of abi.GATHER_POINT_DTYPE (gather_points)
        or an (n, 8) array of 32-bit words holding the same 32-byte records, the host entry; a contiguous (n, 8) float32 / int32 torch
        tensor on this renderer's device goes to the device entry on torch's current stream, no copy made and not waited for, and a
        device tensor comes back.  return_starts: also the generated abi.PathStart records, path (k, s) at k*samples + s -- a numpy
        array of abi.PATH_START_DTYPE, or an (n*samples, 12) float32 tensor -- which radiance() accepts as they are.  Scene, settings,
        statistics and what is left alone: as radiance()."""
        return self._gather("gather", points, int(samples), int(max_depth), None, GATHER_MODES[mode] if isinstance(mode, str) else int(mode), return_starts)

    def gather_sh(self, points, samples, max_depth, order=2, mode="sphere", return_starts=False):
        """SH gather queries on the resident scene (tinsel_hip_gather_sh*): gather()'s paths, point by point and draw by draw, projected
        onto the real spherical harmonics of bands 0 .. order instead of averaged: float32 (n, C, 4), C = (order + 1)^2, entry [k, i, c]
        the mean over s, summed in ascending s, of radiance_c * Y_i(direction) (sh_basis), word 3 zero; no 4 pi or pi folded in -- for
        mode "sphere" 4 pi * the means are the SH coefficients of the incident radiance (sh_irradiance takes those), for "cosine" pi * the
        means those of the cosine-weighted radiance about the normal.  `points`, the host and the device entry, return_starts and what is
        left alone: as gather()."""
        return self._gather("gather_sh", points, int(samples), int(max_depth), int(order), GATHER_MODES[mode] if isinstance(mode, str) else int(mode),
                            return_starts)

    def _gather(self, who, points, samples, max_depth, order, m, return_starts):
        """gather() (order None: tinsel_hip_gather_radiance*, an (n, 4) result) and gather_sh() (tinsel_hip_gather_sh*, (n, C, 4))"""
        entry, lead = ("tinsel_hip_gather_radiance", (m,)) if order is None else ("tinsel_hip_gather_sh", (m, order))
        # (an order out of range is the library's to refuse)
        shape = () if order is None else ((order + 1)**2 if 0 <= order <= abi.GATHER_SH_MAX_ORDER else 1,)
        n, ptr, device, stream = self._records(who, points, 8, "GATHER_POINT_DTYPE")
        if device is not None:
            import torch
            out = torch.empty((n,) + shape + (4,), dtype=torch.float32, device=device)
            starts = torch.empty((n*max(samples, 0), 12), dtype=torch.float32, device=device) if return_starts else None
            if n:
                _check(getattr(self._L, entry + "_device")(self._h, *lead, n, ptr, samples, max_depth, out.data_ptr(),
                                                           starts.data_ptr() if return_starts else None, stream), entry + "_device")
            return (out, starts) if return_starts else out
        out = np.zeros((n,) + shape + (4,), np.float32)
        starts = np.zeros(n*max(samples, 0), abi.PATH_START_DTYPE) if return_starts else None
        _check(getattr(self._L, entry)(self._h, *lead, n, ptr, samples, max_depth, _host_ptr(out),
                                       starts.ctypes.data_as(C.c_void_p) if return_starts and starts.size else None), entry)
        return (out, starts) if return_starts else out

    def trace_camera(self, camera, width, height, time=1.0):
        """tinsel_hip_trace_camera: the closest hit of GenerateRay(i, j) of every pixel (no jitter), an [H, W] record array of abi.RAY_HIT_DTYPE"""
        out = np.zeros((int(height), int(width)), abi.RAY_HIT_DTYPE)
        _check(self._L.tinsel_hip_trace_camera(self._h, C.byref(camera), int(width), int(height), float(time), out.ctypes.data_as(C.c_void_p)),
               "tinsel_hip_trace_camera")
        return out

    def first_hit(self, camera, width, height, time=1.0):
        """The first-hit buffers of a frame: (t [H, W] float32 -- FLT_MAX at a miss, primitive [H, W] int32 -- -1 at a miss,
        normal [H, W, 3] float32 turned towards the camera -- 0 at a miss), from trace_camera."""
        rec = self.trace_camera(camera, width, height, time)
        normal = np.stack([rec["nx"], rec["ny"], rec["nz"]], axis=-1)
        return np.ascontiguousarray(rec["t"]), np.ascontiguousarray(rec["primitive"]), normal

    def first_hit_points(self, camera, width, height, time=1.0, epsilon=RAY_EPSILON):
        """The surface points a frame's camera rays reach first, ready for gather(): (points [H, W, 3] float32 = origin + direction*t moved
        `epsilon` along the normal turned towards the camera, 0 at a miss; t, primitive, normal as first_hit gives them)"""
        t, primitive, normal = self.first_hit(camera, width, height, time)
        origin, d = camera_rays(camera, width, height)
        hit = primitive >= 0
        points = origin + d*np.where(hit, t, 0.0)[..., None] + normal.astype(np.float64)*float(epsilon)
        return np.where(hit[..., None], points, 0.0).astype(np.float32), t, primitive, normal

    def enable_kernel_timing(self, on):
        _check(self._L.tinsel_hip_enable_kernel_timing(self._h, int(on)), "tinsel_hip_enable_kernel_timing")

    def kernel_times(self):
        """{kernel: (launches, sum of their durations in ms, union of their intervals in ms)}; the union is smaller than the sum where a
        call's chunks overlap on two streams.  The record stride is what the LIBRARY says (tinsel_hip_kernel_time_bytes: another build may
        be loaded through TINSEL_HIP_LIB for an A/B); a library too old to say (before round 5: 36- or 40-byte records, nothing to tell them
        apart but the payload) is refused rather than guessed at."""
        if not hasattr(self._L, "tinsel_hip_kernel_time_bytes"):
            raise TinselHipError("%s predates tinsel_hip_kernel_time_bytes: its timing records cannot be read reliably" % LIB_PATH)
        size = self._L.tinsel_hip_kernel_time_bytes()
        if size not in (C.sizeof(abi.KernelTime), C.sizeof(abi.KernelTimeV1)):
            raise TinselHipError("tinsel_hip_kernel_time_bytes() = %d: a record layout this binding does not know" % size)
        raw = (C.c_ubyte * (16 * C.sizeof(abi.KernelTime)))()
        n = self._L.tinsel_hip_kernel_times(self._h, C.cast(raw, C.POINTER(abi.KernelTime)), 16)
        if n < 0:
            _check(n, "tinsel_hip_kernel_times")
        data = bytes(raw)
        T = abi.KernelTime if size == C.sizeof(abi.KernelTime) else abi.KernelTimeV1
        out = {}
        for i in range(n):
            rec = T.from_buffer_copy(data[i*size:(i + 1)*size])
            out[rec.name.decode()] = (rec.launches, rec.total_ms, rec.busy_ms if T is abi.KernelTime else rec.total_ms)
        return out

    def stats(self):
        names = ["rays", "samples", "internal_visits", "tri_tests", "prim_tests", "shadow_rays", "_6", "_7"]
        out = np.zeros(8, np.uint64)
        _check(self._L.tinsel_hip_stats_detail(self._h, out.ctypes.data_as(C.c_void_p)), "tinsel_hip_stats_detail")
        return dict(zip(names, (int(v) for v in out)))

    def batch_radiance(self, passes, height, width):
        """Per-path radiance [passes,H,W,3] of the most recent batch (test hook)."""
        n = passes*height*width
        out = np.empty((n, 4), np.float32)
        got = self._L.tinsel_hip_read_batch_radiance(self._h, out.ctypes.data_as(C.c_void_p), n)
        if got != n:
            raise TinselHipError("batch holds %d paths, wanted %d" % (got, n))
        return out[:, :3].reshape(passes, height, width, 3).copy()

    def leaf(self, op, index, n, out_stride, rows=None, seeds=None, camera=None, width=0, height=0):
        """Test hook: device leaf function `op` on `n` rows (see include/tinsel_hip.h: tinsel_hip_leaf), of the arithmetic arm in force
        (set_arithmetic): the exact build's by default, the tolerance build's after set_arithmetic(abi.ARITH_FAST)."""
        out = np.zeros((n, out_stride), np.float32)
        rp, rs = None, 0
        if rows is not None:
            rows = np.ascontiguousarray(rows, np.float32)
            rp, rs = rows.ctypes.data_as(C.c_void_p), rows.shape[1]
        sp = None
        if seeds is not None:
            seeds = np.ascontiguousarray(seeds, np.uint32)
            sp = seeds.ctypes.data_as(C.c_void_p)
        _check(self._L.tinsel_hip_leaf(self._h, op, index, n, rp, rs, sp, out.ctypes.data_as(C.c_void_p), out_stride,
                                       C.byref(camera) if camera is not None else None, width, height), "tinsel_hip_leaf")
        return out

    def reset_stats(self):
        self._L.tinsel_hip_reset_stats(self._h)

    @property
    def stack_entries(self):
        return self._L.tinsel_hip_stack_entries(self._h)

    def mesh_tree(self, prim):
        """Test hook: the tree of mesh primitive `prim` in force now (tinsel_hip_mesh_tree) -> (Node64 records as a structured
        array with fields lmin, lmax, rmin, rmax [n,3] float32 and left, right uint32, {meta name: int})"""
        meta = (C.c_int * 7)()
        n = self._L.tinsel_hip_mesh_tree(self._h, int(prim), None, 0, meta)
        _check(0 if n >= 0 else -1, "tinsel_hip_mesh_tree")
        dt = np.dtype([("lmin", "<f4", 3), ("lmax", "<f4", 3), ("rmin", "<f4", 3), ("rmax", "<f4", 3),
                       ("left", "<u4"), ("right", "<u4"), ("pad", "<u4", 2)])
        nodes = np.zeros(n, dt)
        got = self._L.tinsel_hip_mesh_tree(self._h, int(prim), nodes.ctypes.data_as(C.c_void_p), n, meta)
        _check(0 if got == n else -1, "tinsel_hip_mesh_tree")
        return nodes, dict(zip(abi.MESH_TREE_META, list(meta)))

    @property
    def nee_per_path(self):
        return self._L.tinsel_hip_nee_per_path(self._h)

    @property
    def walked_prims(self):
        """Primitives whose mesh BVH the dedicated k_walk kernel traverses (0: all meshes are walked inline)."""
        return self._L.tinsel_hip_walked_prims(self._h)

    def walk_tops(self):
        """Node64 records of each walked primitive's tree that k_walk stages into LDS under the tuning in force (tinsel_hip_walk_tops), in
        primitive order; mesh_tree(prim)[1]["topCount"] is the most a primitive can get."""
        out = (C.c_int*8)()
        n = self._L.tinsel_hip_walk_tops(self._h, out, 8)
        _check(min(n, 0), "tinsel_hip_walk_tops")
        return list(out[:n])

    def queue_counts(self, max_bounces=64):
        """(paths alive at the start of each bounce, paths with shadow rays at each bounce) of the last batch."""
        out = (C.c_uint32*(2*max_bounces))()
        n = self._L.tinsel_hip_queue_counts(self._h, out, max_bounces)
        _check(min(n, 0), "tinsel_hip_queue_counts")
        return list(out[:n]), list(out[max_bounces:max_bounces + n])

    def bounce_plan(self):
        """(kind, features) of the fused kernel's last launch: abi.BOUNCE_GENERAL / _FIT_CLOSED / ..., and the abi.BOUNCE_* feature bits
        the scene and the plan asked for."""
        out = (C.c_uint32*2)()
        _check(self._L.tinsel_hip_bounce_plan(self._h, out), "tinsel_hip_bounce_plan")
        return int(out[0]), int(out[1])

    def close(self):
        if self._h:
            self._L.tinsel_hip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HipRendererGroup:
    """`Renderer` (render.h:66-73) over several GPUs of one node: the C-ABI's tinsel_hip_group (one host thread per
    device inside the library, pixel-tile shards, ONE RCCL reduce of the accumulator per read-back)."""

    def __init__(self, scene: Scene, num_gpus: int = 0, tile: int = 64, tuning: "abi.Tuning | None" = None):
        L = load_library()
        self._L = L
        tuning = tuning if tuning is not None else DEFAULT_TUNING
        if tuning is None:
            self._h = L.tinsel_hip_group_create(C.byref(scene.desc), num_gpus, tile)
        else:
            self._h = L.tinsel_hip_group_create_tuned(C.byref(scene.desc), num_gpus, tile, C.byref(tuning))
        if not self._h:
            msg = L.tinsel_hip_last_error()
            raise TinselHipError("tinsel_hip_group_create failed: %s" % (msg.decode() if msg else "?"))
        self.width = self.height = 0

    @property
    def num_gpus(self):
        return self._L.tinsel_hip_group_size(self._h)

    def init(self, width, height):
        _check(self._L.tinsel_hip_group_init(self._h, width, height), "tinsel_hip_group_init")
        self.width, self.height = width, height

    def render(self, camera, options, output=None, passes=1, readback=True):
        if output is None and readback:
            output = np.empty((options.height, options.width, 4), np.float32)
        ptr = output.ctypes.data_as(C.c_void_p) if (readback and output is not None) else None
        _check(self._L.tinsel_hip_group_render(self._h, C.byref(camera), C.byref(options), ptr, passes), "tinsel_hip_group_render")
        return output

    Init = init
    Render = render

    def set_lookahead(self, mode):
        """Trace and reduce the next calls while this call's image is copied out (tinsel_hip_group_set_lookahead); images unchanged.
        mode: abi.LOOKAHEAD_OFF / ON / PIN_OUTPUT (or a bool)."""
        _check(self._L.tinsel_hip_group_set_lookahead(self._h, int(mode)), "tinsel_hip_group_set_lookahead")

    def present(self, options, nlm_width=0, nlm_falloff=200.0):
        out = np.empty((self.height, self.width, 4), np.float32)
        _check(self._L.tinsel_hip_group_present(self._h, C.byref(options), int(nlm_width), float(nlm_falloff), out.ctypes.data_as(C.c_void_p)),
               "tinsel_hip_group_present")
        return out

    def member_stats(self, rank):
        """rays / samples counters of member `rank` (tinsel_hip_stats_detail on its renderer)."""
        m = self._L.tinsel_hip_group_member(self._h, rank)
        out = np.zeros(8, np.uint64)
        _check(self._L.tinsel_hip_stats_detail(m, out.ctypes.data_as(C.c_void_p)), "tinsel_hip_stats_detail")
        return {"rays": int(out[0]), "samples": int(out[1]), "shadow_rays": int(out[5])}

    def close(self):
        if self._h:
            self._L.tinsel_hip_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


UBENCH_COPY, UBENCH_GATHER_BEYOND_CACHE, UBENCH_GATHER_TREE, UBENCH_GATHER_L2 = 0, 1, 2, 3


def ubench(kind, nbytes, steps=64, device=0):
    """tinsel_hip_ubench: (milliseconds, units) of one timed launch -- units = bytes moved (copy) or 64-B records visited."""
    L = load_library()
    ms, units = C.c_double(0.0), C.c_double(0.0)
    _check(L.tinsel_hip_ubench(int(device), int(kind), int(nbytes), int(steps), C.byref(ms), C.byref(units)), "tinsel_hip_ubench")
    return ms.value, units.value


def plan_regions(slots, num_cus=256, nee_per_path=1, fused=True):
    """tinsel_hip_plan_regions: dict of how a batch of `slots` path slots would be cut (host arithmetic only, no GPU needed)."""
    L = load_library()
    out = (C.c_uint*6)()
    _check(L.tinsel_hip_plan_regions(int(slots), int(num_cus), int(nee_per_path), 1 if fused else 0, out), "tinsel_hip_plan_regions")
    return dict(zip(("num_regions", "region_len", "big_regions", "short_len", "grid", "max_regions"), (int(v) for v in out)))


def selftest_sort(keys, begin_bit=0, end_bit=64, device=0):
    """tinsel_hip_selftest_sort: the library's stable LSD radix sort of uint64 keys by their bits [begin_bit, end_bit); returns the sorted copy"""
    L = load_library()
    out = np.ascontiguousarray(keys, np.uint64).copy()
    _check(L.tinsel_hip_selftest_sort(int(device), out.ctypes.data_as(C.c_void_p), out.size, int(begin_bit), int(end_bit)), "tinsel_hip_selftest_sort")
    return out


def selftest_scan(values, device=0):
    """tinsel_hip_selftest_scan: the library's exclusive prefix sum of int32 values"""
    L = load_library()
    a = np.ascontiguousarray(values, np.int32)
    out = np.empty_like(a)
    _check(L.tinsel_hip_selftest_scan(int(device), a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), a.size), "tinsel_hip_selftest_scan")
    return out


def selftest_accumulate(radiance, accum, pass_seeds, filter, clamp, choice=abi.ACCUMULATE_AUTO, form=abi.ACCUMULATE_FORM_AUTO, device=0):
    """tinsel_hip_selftest_accumulate: radiance[passes, H, W, 4] added to a copy of accum[H, W, 4] by the launch a render of such a frame makes;
    filter = (type, width, falloff, offset).  Returns (the new accumulator, the form that ran: abi.ACCUMULATE_RAN_*)."""
    L = load_library()
    rad = np.ascontiguousarray(radiance, np.float32)
    out = np.array(accum, np.float32, order="C")
    seeds = np.ascontiguousarray(pass_seeds, np.uint32)
    passes, H, W = rad.shape[0], rad.shape[1], rad.shape[2]
    if rad.shape != (passes, H, W, 4) or out.shape != (H, W, 4) or seeds.shape != (passes,):
        raise ValueError("selftest_accumulate: radiance[passes, H, W, 4], accum[H, W, 4], pass_seeds[passes]")
    ran = C.c_int(-1)
    _check(L.tinsel_hip_selftest_accumulate(int(device), W, H, int(filter[0]), float(filter[1]), float(filter[2]), float(filter[3]), float(clamp),
                                            _host_ptr(seeds), passes, _host_ptr(rad), _host_ptr(out), int(choice), int(form), C.byref(ran)),
           "tinsel_hip_selftest_accumulate")
    return out, ran.value


def selftest_arith(op, variant=-1, device=0):
    """tinsel_hip_selftest_arith: (counts[4 + 256 by exponent field], first_bad) of the exhaustive 2^32-input comparison of a reciprocal (op 0) /
    square-root (op 1) sequence with the compiler's IEEE expansion; variant -1 = the one the library is built with."""
    L = load_library()
    counts, first = (C.c_ulonglong*260)(), C.c_uint(0)
    _check(L.tinsel_hip_selftest_arith(int(device), int(op), int(variant), counts, C.byref(first)), "tinsel_hip_selftest_arith")
    return [int(c) for c in counts], int(first.value)


def create_gpu_renderer(scene: Scene, device: int = 0, tuning: "abi.Tuning | None" = None) -> HipRenderer:
    """`Renderer* CreateGpuRenderer(const Scene*)` (render.h:79); `tuning`: an abi.Tuning (tinsel_hip_create_tuned), None = the defaults."""
    return HipRenderer(scene, device, tuning)


class use_tuning:
    """`with use_tuning(walk_min_tris=0, small_mesh_bytes=0): ...` -- renderers created inside the block without an explicit tuning get
    this one (DEFAULT_TUNING above).  Also usable as `use_tuning(...).__enter__()` / pytest's monkeypatch.setattr(renderer, "DEFAULT_TUNING", ..)."""

    def __init__(self, tuning=None, **fields):
        self.tuning = (tuning if tuning is not None else abi.Tuning()).replace(**fields)

    def __enter__(self):
        global DEFAULT_TUNING
        self._was = DEFAULT_TUNING
        DEFAULT_TUNING = self.tuning
        return self.tuning

    def __exit__(self, *exc):
        global DEFAULT_TUNING
        DEFAULT_TUNING = self._was
        return False


def resolve(accum):
    """Consumer-side normalisation of main.cpp:262-268: rgb / w (0 where w == 0)."""
    w = accum[..., 3:4]
    return np.where(w > 0, accum[..., :3] / np.where(w > 0, w, 1.0), 0.0)

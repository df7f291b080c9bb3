"""tinsel_amd -- MI355X (gfx950) streaming path tracer behind Tinsel's Renderer API.

Only what the hot path needs: `csrc/` (hand-written HIP kernels + the C-ABI of
include/tinsel_hip.h), `renderer.py` (host mirror of render.h:66-79), `abi.py`
(ctypes PODs), `build.py` (hipcc driver), `distributed.py` (pixel-tile shard + reduce).
"""
from . import abi  # noqa: F401
from .renderer import HipRenderer, HipRendererGroup, Scene, TinselHipError, camera_rays, create_gpu_renderer, crop_sample_map, cube_cameras, default_light_groups, denoise_params, depth_contributions, feature_images, feature_mask, gather_points, load_library, matte, merge_id_mattes, orbit_cameras, plan_regions, plan_sample_map, plan_views, rank_id_lists, relight, resolve, rng_state, selftest_accumulate, selftest_arith, selftest_scan, selftest_sort, sh_basis, sh_irradiance, ubench, use_tuning  # noqa: F401

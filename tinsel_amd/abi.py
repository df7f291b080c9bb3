"""ctypes mirrors of include/tinsel_hip.h (which mirrors the reference PODs).

Reference layouts: Vec3 maths.h:214, Transform maths.h:575, BVHNode bvh.h:9,
Camera scene.h:11, Material scene.h:45, MeshGeometry scene.h:119,
Primitive scene.h:138, Filter render.h:13, Options render.h:50.
"""
import ctypes as C


class Vec3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]

    def __iter__(self):
        return iter((self.x, self.y, self.z))


class Vec4(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("w", C.c_float)]

    def __iter__(self):
        return iter((self.x, self.y, self.z, self.w))


class Transform(C.Structure):
    _fields_ = [("p", Vec3), ("r", Vec4), ("s", C.c_float)]


class BVHNode(C.Structure):
    _fields_ = [("lower", Vec3), ("upper", Vec3), ("left_index", C.c_uint32), ("right_index_leaf", C.c_uint32)]


class Node64(C.Structure):
    """tn_scene.h Node64: one internal node of a mesh tree as the kernels read it (tinsel_hip_mesh_tree) -- both children's boxes,
    then the child refs (bit 31 set: a leaf, the low bits its triangle index; clear: an internal node's index)"""
    _fields_ = [("lmin", C.c_float * 3), ("lmax", C.c_float * 3), ("rmin", C.c_float * 3), ("rmax", C.c_float * 3),
                ("left", C.c_uint32), ("right", C.c_uint32), ("_pad", C.c_uint32 * 2)]


LEAF_BIT = 0x80000000
MESH_TREE_META = ("root", "numInternal", "numTris", "stackNeed", "topCount", "twoLeaves", "inArena")


class Camera(C.Structure):
    _fields_ = [("position", Vec3), ("rotation", Vec4), ("fov", C.c_float),
                ("shutter_start", C.c_float), ("shutter_end", C.c_float)]


class Texture(C.Structure):
    _fields_ = [("data", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32),
                ("depth", C.c_int32), ("_pad", C.c_int32)]


class Material(C.Structure):
    _fields_ = [("emission", Vec3), ("color", Vec3), ("absorption", Vec3),
                ("eta", C.c_float), ("metallic", C.c_float), ("subsurface", C.c_float),
                ("specular", C.c_float), ("roughness", C.c_float), ("specular_tint", C.c_float),
                ("anisotropic", C.c_float), ("sheen", C.c_float), ("sheen_tint", C.c_float),
                ("clearcoat", C.c_float), ("clearcoat_gloss", C.c_float), ("transmission", C.c_float),
                ("_pad0", C.c_int32), ("bump_map", Texture), ("bump", C.c_float), ("bump_tile", Vec3)]


class MeshGeometry(C.Structure):
    _fields_ = [("positions", C.c_void_p), ("normals", C.c_void_p), ("indices", C.c_void_p),
                ("nodes", C.c_void_p), ("cdf", C.c_void_p),
                ("num_vertices", C.c_int32), ("num_indices", C.c_int32), ("num_nodes", C.c_int32),
                ("area", C.c_float), ("id", C.c_uint64)]


class _Sphere(C.Structure):
    _fields_ = [("radius", C.c_float)]


class _Plane(C.Structure):
    _fields_ = [("plane", C.c_float * 4)]


class _Geo(C.Union):
    _fields_ = [("sphere", _Sphere), ("plane", _Plane), ("mesh", MeshGeometry)]


class Primitive(C.Structure):
    _fields_ = [("start_transform", Transform), ("end_transform", Transform),
                ("type", C.c_int32), ("_pad0", C.c_int32), ("geo", _Geo),
                ("material", Material), ("light_samples", C.c_int32), ("_pad1", C.c_int32)]


class Filter(C.Structure):
    _fields_ = [("type", C.c_int32), ("width", C.c_float), ("falloff", C.c_float), ("offset", C.c_float)]


class Options(C.Structure):
    _fields_ = [("mode", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("filter", Filter),
                ("exposure", C.c_float), ("limit", C.c_float), ("clamp", C.c_float),
                ("max_depth", C.c_int32), ("max_samples", C.c_int32)]

    def copy(self):
        o = Options()
        C.memmove(C.byref(o), C.byref(self), C.sizeof(Options))
        return o


class SceneDesc(C.Structure):
    _fields_ = [("primitives", C.c_void_p), ("num_primitives", C.c_int32), ("num_bvh_nodes", C.c_int32),
                ("bvh_nodes", C.c_void_p), ("sky_horizon", Vec3), ("sky_zenith", Vec3),
                ("probe_valid", C.c_int32), ("probe_width", C.c_int32), ("probe_height", C.c_int32),
                ("_pad", C.c_int32), ("probe_data", C.c_void_p), ("probe_pdf_x", C.c_void_p),
                ("probe_cdf_x", C.c_void_p), ("probe_pdf_y", C.c_void_p), ("probe_cdf_y", C.c_void_p)]


class PackHeader(C.Structure):
    _fields_ = [("magic", C.c_char * 8), ("version", C.c_uint32), ("num_primitives", C.c_uint32),
                ("num_bvh_nodes", C.c_uint32), ("num_meshes", C.c_uint32), ("total_bytes", C.c_uint64),
                ("off_primitives", C.c_uint64), ("off_bvh_nodes", C.c_uint64), ("off_probe_data", C.c_uint64),
                ("off_probe_pdf_x", C.c_uint64), ("off_probe_cdf_x", C.c_uint64),
                ("off_probe_pdf_y", C.c_uint64), ("off_probe_cdf_y", C.c_uint64),
                ("probe_width", C.c_int32), ("probe_height", C.c_int32),
                ("sky_horizon", Vec3), ("sky_zenith", Vec3), ("camera", Camera), ("options", Options),
                ("_reserved", C.c_uint8 * 48)]


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("launches", C.c_uint32), ("total_ms", C.c_float), ("busy_ms", C.c_float)]


class Ray(C.Structure):
    """tinsel_ray: origin, the time that poses moving primitives, direction (used as given), tmax (occlusion queries)"""
    _fields_ = [("ox", C.c_float), ("oy", C.c_float), ("oz", C.c_float), ("time", C.c_float),
                ("dx", C.c_float), ("dy", C.c_float), ("dz", C.c_float), ("tmax", C.c_float)]


class RayHit(C.Structure):
    """tinsel_ray_hit: closest t > 0, its primitive (-1: a miss, t = FLT_MAX), the normal turned towards the ray"""
    _fields_ = [("t", C.c_float), ("primitive", C.c_int32), ("nx", C.c_float), ("ny", C.c_float), ("nz", C.c_float),
                ("reserved", C.c_uint32 * 3)]


# the same records as numpy dtypes: an (n, 8) float32 array viewed as RAY_DTYPE is a tinsel_ray[n]
RAY_DTYPE = [("ox", "<f4"), ("oy", "<f4"), ("oz", "<f4"), ("time", "<f4"), ("dx", "<f4"), ("dy", "<f4"), ("dz", "<f4"), ("tmax", "<f4")]
RAY_HIT_DTYPE = [("t", "<f4"), ("primitive", "<i4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("reserved", "<u4", (3,))]
QUERY_CLOSEST, QUERY_OCCLUDED = 0, 1


class PathStart(C.Structure):
    """tinsel_path_start: the ray a path starts with (direction used as given; PathTrace expects unit length), its shutter time, and the
    two words of the reference's Random when PathTrace is entered (tinsel_amd.rng_state); reserved words are ignored"""
    _fields_ = [("ox", C.c_float), ("oy", C.c_float), ("oz", C.c_float), ("time", C.c_float),
                ("dx", C.c_float), ("dy", C.c_float), ("dz", C.c_float), ("reserved0", C.c_float),
                ("rng1", C.c_uint32), ("rng2", C.c_uint32), ("reserved1", C.c_uint32), ("reserved2", C.c_uint32)]


# an (n, 12) array of 32-bit words viewed as PATH_START_DTYPE is a tinsel_path_start[n]
PATH_START_DTYPE = [("ox", "<f4"), ("oy", "<f4"), ("oz", "<f4"), ("time", "<f4"), ("dx", "<f4"), ("dy", "<f4"), ("dz", "<f4"), ("reserved0", "<f4"),
                    ("rng1", "<u4"), ("rng2", "<u4"), ("reserved1", "<u4"), ("reserved2", "<u4")]


class GatherPoint(C.Structure):
    """tinsel_gather_point: a surface point a gather query starts `samples` paths from -- position (the origin as given), shutter time,
    normal (unit length, used as given) and the seed of its first sample (sample s draws from Random(seed + s))"""
    _fields_ = [("px", C.c_float), ("py", C.c_float), ("pz", C.c_float), ("time", C.c_float),
                ("nx", C.c_float), ("ny", C.c_float), ("nz", C.c_float), ("seed", C.c_uint32)]


# an (n, 8) array of 32-bit words viewed as GATHER_POINT_DTYPE is a tinsel_gather_point[n]
GATHER_POINT_DTYPE = [("px", "<f4"), ("py", "<f4"), ("pz", "<f4"), ("time", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("seed", "<u4")]
GATHER_COSINE, GATHER_SPHERE = 0, 1
GATHER_SH_MAX_ORDER = 2       # tinsel_hip_gather_sh*: bands 0 .. order, (order + 1)^2 coefficients per channel
# tinsel_hip_render_features*: the planes a call asks for, by bit; the output holds them in ascending bit order (FEATURE_NAMES' order)
FEATURE_ALBEDO, FEATURE_NORMAL, FEATURE_DEPTH = 1, 2, 4
FEATURE_NAMES = ("albedo", "normal", "depth")
# tinsel_hip_render_id_mattes*: the id of a path that left the scene, the id of an unused slot, the most slots a call takes
ID_MISS, ID_EMPTY, ID_MAX_SLOTS = -1, -2, 8
# tinsel_hip_render_light_groups*: the most planes a call takes
MAX_LIGHT_GROUPS = 8
# tinsel_hip_render_views*: the most views a call takes, and its flags
MAX_VIEWS = 4096
VIEWS_ADD, VIEWS_ACCUMULATE_SINGLY = 1, 2
# tinsel_hip_render_depth_planes*: the most planes a call takes, the deepest plane, its flags, and the entries' signatures -- renderer,
# camera, options, pass_begin, passes, num_planes, depths (host int32 [num_planes]), flags, out (, stream)
MAX_DEPTH_PLANES = 16
MAX_PLANE_DEPTH = 64
DEPTH_PLANES_ADD, DEPTH_PLANES_ACCUMULATE_SINGLY = 1, 2
RENDER_DEPTH_PLANES_ARGTYPES = [C.c_void_p, C.POINTER(Camera), C.POINTER(Options), C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
RENDER_DEPTH_PLANES_DEVICE_ARGTYPES = RENDER_DEPTH_PLANES_ARGTYPES + [C.c_void_p]
# tinsel_hip_render_sample_map*: the largest count of a pixel (a uint16), its flag, and the entries' signatures -- renderer, camera,
# options, pass_begin, counts (host uint16 [H*W]), flags, out (, stream); slot_limit, width, height, counts, out4
SAMPLE_MAP_MAX = 65535
SAMPLES_ADD = 1
RENDER_SAMPLE_MAP_ARGTYPES = [C.c_void_p, C.POINTER(Camera), C.POINTER(Options), C.c_uint32, C.c_void_p, C.c_uint, C.c_void_p]
RENDER_SAMPLE_MAP_DEVICE_ARGTYPES = RENDER_SAMPLE_MAP_ARGTYPES + [C.c_void_p]
PLAN_SAMPLE_MAP_ARGTYPES = [C.c_ulonglong, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_ulonglong)]


class DenoiseParams(C.Structure):
    """tinsel_hip_denoise_params: the search window's radius (1 .. 8), AverageFilter's radius (0 .. 4), the coefficients of the colour,
    albedo, normal and depth terms of the exponent (finite, >= 0), demodulation by the albedo (0 | 1; needs the albedo plane) and the
    floor of its divisor (> 0).  tinsel_amd.denoise_params(**fields) starts from the library's defaults."""
    _fields_ = [("radius", C.c_int32), ("patch_radius", C.c_int32),
                ("k_color", C.c_float), ("k_albedo", C.c_float), ("k_normal", C.c_float), ("k_depth", C.c_float),
                ("demodulate", C.c_int32), ("albedo_floor", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class KernelTimeV1(C.Structure):
    """tinsel_kernel_time as libraries built before round 4 wrote it (no busy_ms): renderer.HipRenderer.kernel_times"""
    _fields_ = [("name", C.c_char * 32), ("launches", C.c_uint32), ("total_ms", C.c_float)]


# tinsel_hip_bounce_plan: k_bounce's kinds and the feature bits asked of it (include/tinsel_hip.h TINSEL_BOUNCE_*)
BOUNCE_GENERAL, BOUNCE_COUNT, BOUNCE_FIT_CLOSED, BOUNCE_FIT_DEFERRED = 0, 1, 2, 3
BOUNCE_MEDIA, BOUNCE_PROBE, BOUNCE_MOTION, BOUNCE_MESH_WALK, BOUNCE_SPHERE = 1, 2, 4, 8, 16
BOUNCE_TRANSMISSION, BOUNCE_POOLS, BOUNCE_SHARE, BOUNCE_SORT, BOUNCE_ROULETTE = 32, 64, 128, 256, 512


# tinsel_hip_bake_status / tinsel_hip_install_baked (include/tinsel_hip.h TINSEL_BAKE_*)
BAKE_OFF, BAKE_NOT_BAKEABLE, BAKE_NO_COMPILER, BAKE_COMPILED, BAKE_FROM_CACHE, BAKE_STALE, BAKE_NONE, BAKE_LDS_REFUSED = 0, 1, 2, 3, 4, 5, 6, 7
BAKE_AUTO_MIN_PATHS = 64 << 20      # auto bakes at a reservation of one default batch (64 Mi path slots) or more


class Tuning(C.Structure):
    """tinsel_hip_tuning (include/tinsel_hip.h): every choice between two code paths of the library as one plain struct.  Tuning() holds
    the defaults ("the library decides"); Tuning(walk_min_tris=0, small_mesh_bytes=0) overrides fields.  Nothing is read from the
    environment."""
    _fields_ = [("struct_bytes", C.c_uint32),
                ("flat_scan", C.c_int32), ("lds_scene", C.c_int32), ("walk", C.c_int32), ("inline_max_tris", C.c_int32), ("walk_min_tris", C.c_int32),
                ("small_mesh_bytes", C.c_int64), ("arena_lds_limit", C.c_int64),
                ("batch_paths", C.c_int64), ("grid_mult", C.c_int32), ("bounce_share", C.c_int32), ("repack", C.c_int32),
                ("tail_split", C.c_int32), ("tail_share", C.c_float), ("tail_divide", C.c_int32),
                ("shade_sorted", C.c_int32), ("overlap", C.c_int32), ("scene_walk", C.c_int32), ("swalk_lds", C.c_int32), ("accumulate", C.c_int32),
                ("walk_block", C.c_int32), ("walk_single", C.c_int32), ("walk_lds_stack", C.c_int32), ("walk_refill_min", C.c_int32), ("walk_leaf_min", C.c_int32),
                ("walk_grid_mult", C.c_int32), ("quads_in_scan", C.c_int32), ("bounce_fit", C.c_int32), ("plane_pairs", C.c_int32)]
    # `bounce_bake` (-1 auto | 0 never | 1 always: baked instances, include/tinsel_hip.h tinsel_hip_set_bounce_bake) travels with a Tuning in
    # this binding -- Tuning(bounce_bake=0), set_tuning(bounce_bake=1), bench.py --tuning -- but is NOT a field of the C struct, whose layout
    # stays as it is: the renderer hands it to the library through its own setter (HipRenderer._apply_bake_mode)
    BINDING_FIELDS = ("bounce_bake",)
    bounce_bake = -1        # (the default of an instance that was not made by __init__, e.g. from_buffer_copy)
    CREATE_FIELDS = ("flat_scan", "lds_scene", "walk", "inline_max_tris", "walk_min_tris", "small_mesh_bytes", "arena_lds_limit")
    _DEFAULTS = dict(flat_scan=-1, lds_scene=-1, walk=-1, inline_max_tris=-1, walk_min_tris=-1, small_mesh_bytes=-1, arena_lds_limit=-1,
                     batch_paths=0, grid_mult=0, bounce_share=-1, repack=-1, tail_split=-1, tail_share=0.0, tail_divide=4,
                     shade_sorted=-1, overlap=-1, scene_walk=-1, swalk_lds=-1, accumulate=0,
                     walk_block=0, walk_single=-1, walk_lds_stack=-1, walk_refill_min=0, walk_leaf_min=0, walk_grid_mult=0, quads_in_scan=-1, bounce_fit=-1, plane_pairs=-1, bounce_bake=-1)

    def __init__(self, **over):
        super().__init__()
        self.struct_bytes = C.sizeof(Tuning)
        for k, v in self._DEFAULTS.items():
            setattr(self, k, v)
        for k, v in over.items():
            if k not in self._DEFAULTS:
                raise TypeError("tinsel_hip_tuning has no field %r" % k)
            setattr(self, k, v)

    def replace(self, **over):
        t = Tuning(**{k: getattr(self, k) for k in self._DEFAULTS})
        for k, v in over.items():
            if k not in self._DEFAULTS:
                raise TypeError("tinsel_hip_tuning has no field %r" % k)
            setattr(t, k, v)
        return t

    def as_dict(self):
        return {k: getattr(self, k) for k in self._DEFAULTS}


ACCUMULATE_AUTO, ACCUMULATE_TILED, ACCUMULATE_WIDE, ACCUMULATE_PIPED, ACCUMULATE_FULL_WINDOW = 0, 1, 2, 3, 4
# tinsel_hip_selftest_accumulate: the form asked for, the form that ran
ACCUMULATE_FORM_AUTO, ACCUMULATE_FORM_FULL_WINDOW, ACCUMULATE_FORM_SUPPORT = 0, 1, 2
ACCUMULATE_RAN_UNTILED, ACCUMULATE_RAN_TILED, ACCUMULATE_RAN_WIDE, ACCUMULATE_RAN_PIPED, ACCUMULATE_RAN_SUPPORT_TILED, ACCUMULATE_RAN_SUPPORT_WIDE = 0, 1, 2, 3, 4, 5
SELFTEST_ACCUMULATE_ARGTYPES = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                C.c_int, C.c_int, C.POINTER(C.c_int)]


def accumulate_arg_zero(offset):
    """The expf argument at and below which Filter::Gaussian's weight max(0, expf(a) - offset) is +0 by construction: log(offset) - 1e-6 in
    double, rounded down to float (launch_accumulate's rule, tn_host_batch.h)."""
    import math
    import numpy as np
    z = math.log(float(np.float32(offset))) - 1e-6
    f = np.float32(z)
    if float(f) > z:
        f = np.nextafter(f, np.float32(-np.inf))
    return f


def accumulate_takes_support_form(filter_type, width, falloff, offset):
    """launch_accumulate's rule (accumulate_support_rule, tn_host_batch.h) restated: does k_accumulate_tiled run in its support form for this filter?"""
    import numpy as np
    width, falloff, offset = np.float32(width), np.float32(falloff), np.float32(offset)
    if filter_type == FILTER_BOX or not (offset > 0 and np.isfinite(offset)) or not (falloff > 0 and np.isfinite(falloff)) or not (0 < width <= 1):
        return False
    return bool(-falloff <= accumulate_arg_zero(offset))
COMM_ID_BYTES = 128
MODE_NORMALS, MODE_COMPLEXITY, MODE_PATHTRACE = 0, 1, 2
BVH_REFERENCE, BVH_LBVH, BVH_PLOC = 0, 1, 2
SCENE_BVH_NODES, SCENE_BVH_DEVICE = 0, 1
ARITH_EXACT, ARITH_FAST = 0, 1
PROBE_CDF, PROBE_ALIAS = 0, 1
LOOKAHEAD_OFF, LOOKAHEAD_ON, LOOKAHEAD_PIN_OUTPUT = 0, 1, 2
FILTER_BOX, FILTER_GAUSSIAN = 0, 1
GEOM_SPHERE, GEOM_PLANE, GEOM_MESH = 0, 1, 2
PIPELINE_WAVEFRONT, PIPELINE_MEGAKERNEL, PIPELINE_WAVEFRONT_SPLIT, PIPELINE_AUTO, PIPELINE_WAVEFRONT_PAIRED = 0, 1, 2, 3, 4

assert C.sizeof(Transform) == 32 and C.sizeof(BVHNode) == 32 and C.sizeof(Camera) == 40 and C.sizeof(Node64) == 64
assert C.sizeof(Material) == 128 and C.sizeof(MeshGeometry) == 64 and C.sizeof(Primitive) == 272
assert C.sizeof(Filter) == 16 and C.sizeof(Options) == 48 and C.sizeof(PackHeader) == 256
assert C.sizeof(Ray) == 32 and C.sizeof(RayHit) == 32 and C.sizeof(DenoiseParams) == 32
assert Primitive.geo.offset == 72 and Primitive.material.offset == 136 and Primitive.light_samples.offset == 264

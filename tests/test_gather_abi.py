"""CPU tests of the gather-query boundary (tinsel_hip_gather_radiance / _device): the 32-byte point record in the header, the ctypes mirror
and the numpy dtype, the exported and bound entries, the two kernels in the library under both arithmetic contracts, the refusals that
need no GPU, the point-array helper's seeds, the camera-ray helper and the headless options."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tinsel_amd
from tinsel_amd import abi, headless
from tests import oracle_api as oa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "tinsel_hip.h")).read()


def test_the_point_is_32_bytes_in_the_header_the_mirror_and_the_dtype():
    assert re.search(r"static_assert\(sizeof\(tinsel_gather_point\) == 32", HEADER)
    m = re.search(r"typedef struct tinsel_gather_point\s*\{([^}]*)\}", HEADER)
    fields, offset = [], 0
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        assert ctype in ("float", "uint32_t")
        for name in names.split(","):
            fields.append((name.strip(), ctype, offset))
            offset += 4
    assert offset == 32 and len(fields) == 8
    assert C.sizeof(abi.GatherPoint) == 32 and np.dtype(abi.GATHER_POINT_DTYPE).itemsize == 32
    dt = np.dtype(abi.GATHER_POINT_DTYPE)
    mirror = [(n, "float" if t is C.c_float else "uint32_t", getattr(abi.GatherPoint, n).offset) for n, t in abi.GatherPoint._fields_]
    numpy = [(n, "float" if dt.fields[n][0] == np.dtype("<f4") else "uint32_t", dt.fields[n][1]) for n in dt.names]
    assert fields == mirror == numpy
    assert [f[0] for f in fields] == ["px", "py", "pz", "time", "nx", "ny", "nz", "seed"] and fields[7][1] == "uint32_t"
    assert re.search(r"#define TINSEL_GATHER_COSINE 0\b", HEADER) and re.search(r"#define TINSEL_GATHER_SPHERE 1\b", HEADER)
    assert (abi.GATHER_COSINE, abi.GATHER_SPHERE) == (0, 1)
    # an (n, 8) array of 32-bit words IS a tinsel_gather_point[n]
    v = np.arange(16, dtype=np.uint32).reshape(2, 8).view(abi.GATHER_POINT_DTYPE)
    assert v["seed"][1, 0] == 15 and v["time"].view(np.uint32)[0, 0] == 3 and v["nx"].view(np.uint32)[1, 0] == 12


def test_the_entries_are_exported_and_bound():
    L = tinsel_amd.load_library()
    for name in ("tinsel_hip_gather_radiance", "tinsel_hip_gather_radiance_device"):
        assert hasattr(L, name) and name in tinsel_amd.renderer.EXPORTED_SYMBOLS
        assert re.search(r"\bint %s\(tinsel_hip\* r, int mode, long long n, const tinsel_gather_point\* \w+, int samples, int max_depth,\s*"
                         r"float\* \w+, tinsel_path_start\* \w+" % name, HEADER)
    host, dev = L.tinsel_hip_gather_radiance.argtypes, L.tinsel_hip_gather_radiance_device.argtypes
    assert len(host) == 8 and len(dev) == 9 and dev[:8] == host
    assert host[1] is C.c_int and host[2] is C.c_longlong and host[4] is C.c_int and host[5] is C.c_int
    assert all(host[k] is C.c_void_p for k in (0, 3, 6, 7)) and dev[8] is C.c_void_p
    assert callable(tinsel_amd.HipRenderer.gather) and callable(tinsel_amd.gather_points)


def test_the_kernels_are_in_the_library_under_both_arithmetic_contracts():
    blob = open(tinsel_amd.renderer.LIB_PATH, "rb").read()
    for ns in (b"_ZN2tn", b"_ZN7tn_fast"):
        assert ns + b"17k_generate_gatherE" in blob and ns + b"15k_gather_reduceE" in blob
    launch = open(os.path.join(ROOT, "tinsel_amd", "csrc", "tn_launch.h")).read()
    assert re.search(r"X\(PK_GENERATE_GATHER,\s+kBlock, 0, GENERATE_GATHER,\s*k_generate_gather\)", launch)
    assert re.search(r"X\(PK_GATHER_REDUCE,\s+kBlock, 0, GATHER_REDUCE,\s*k_gather_reduce\)", launch)
    layout = open(os.path.join(ROOT, "tinsel_amd", "csrc", "tn_host_layout.h")).read()
    assert '"k_generate_gather"' in layout and '"k_gather_reduce"' in layout


def test_refusals_that_need_no_gpu():
    """(the arguments are judged before the renderer is looked at: a handle that is only non-null will do)"""
    L = tinsel_amd.load_library()
    points = np.zeros((4, 8), np.float32)
    out = np.full(4*16, 0xa5, np.uint8)
    pp, op = points.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    handle = C.create_string_buffer(1 << 16)
    host = lambda *a: L.tinsel_hip_gather_radiance(*a, None)
    dev = lambda *a: L.tinsel_hip_gather_radiance_device(*a, None, None)
    for fn, own in ((host, b"gather_radiance:"), (dev, b"gather_radiance_device:")):
        cases = [
            (None, 0, 4, pp, 8, 4, op),             # null renderer
            (handle, -1, 4, pp, 8, 4, op),          # mode out of range
            (handle, 2, 4, pp, 8, 4, op),
            (handle, 0, -1, pp, 8, 4, op),          # n < 0
            (handle, 0, 2**31, pp, 8, 4, op),       # n >= 2^31
            (handle, 0, 4, pp, 0, 4, op),           # samples outside [1, 65536]
            (handle, 0, 4, pp, 65537, 4, op),
            (handle, 1, 4, pp, 8, 0, op),           # max_depth < 1
            (handle, 0, 4, None, 8, 4, op),         # a null array with n > 0
            (handle, 1, 4, pp, 8, 4, None),
        ]
        for case in cases:
            assert L.tinsel_hip_init(None, 0, 0) == -1 and L.tinsel_hip_last_error().startswith(b"init:")      # another entry's text in between
            assert fn(*case) == -1, case
            assert L.tinsel_hip_last_error().startswith(own), L.tinsel_hip_last_error()
            assert (out == 0xa5).all() and not points.any()


def test_gather_points_lays_out_seeds_as_documented():
    rng = np.random.default_rng(5)
    pos, nrm = rng.normal(size=(7, 3)).astype(np.float32), rng.normal(size=(7, 3)).astype(np.float32)
    pts = tinsel_amd.gather_points(pos, nrm, 67)
    assert pts.dtype == np.dtype(abi.GATHER_POINT_DTYPE) and pts.shape == (7,)
    assert pts["seed"].tolist() == [k*67 for k in range(7)] and (pts["time"] == 1.0).all()
    w = pts.view(np.float32).reshape(7, 8)
    assert np.array_equal(w[:, 0:3], pos) and np.array_equal(w[:, 4:7], nrm)
    # the base seed, wrapping in 32 bits; per-point times
    times = np.linspace(0.0, 1.0, 7).astype(np.float32)
    pts = tinsel_amd.gather_points(pos, nrm, 256, time=times, base_seed=2**32 - 300)
    assert pts["seed"].tolist() == [(2**32 - 300 + k*256) % 2**32 for k in range(7)] and np.array_equal(pts["time"], times)
    # the caller's own seeds
    own = np.array([9, 8, 7, 6, 5, 4, 2**32 - 1], np.uint32)
    assert np.array_equal(tinsel_amd.gather_points(pos, nrm, 4, seeds=own)["seed"], own)
    assert tinsel_amd.gather_points(np.zeros((0, 3)), np.zeros((0, 3)), 4).shape == (0,)


def test_camera_rays_are_unit_and_look_down_the_cameras_axis():
    cam = abi.Camera()
    cam.position.x, cam.position.y, cam.position.z = 1.0, 2.0, 3.0
    cam.rotation.w = 1.0                                        # identity: the camera looks down -z, +y up
    cam.fov = np.float32(np.pi/2)
    o, d = tinsel_amd.camera_rays(cam, 8, 6)
    assert o.tolist() == [1.0, 2.0, 3.0] and d.shape == (6, 8, 3)
    assert np.allclose(np.linalg.norm(d, axis=-1), 1.0, atol=1e-12)
    assert np.allclose(d[3, 4], [0.0, 0.0, -1.0], atol=1e-7)    # raster (4, 3) is the frame's centre
    assert d[0, 0, 0] < 0 < d[0, 0, 1] and d[5, 7, 0] > 0       # pixel (0, 0) is up and to the left
    assert np.isclose(d[3, 0, 0]/-d[3, 0, 2], -8.0/6.0, atol=1e-6)     # tan(fov/2)*aspect at the left edge (tan is 1 to float32's pi)
    # a quarter turn about +y (q = (0, sin 45, 0, cos 45)) turns -z into -x
    cam.rotation.y, cam.rotation.w = np.sqrt(0.5), np.sqrt(0.5)
    assert np.allclose(tinsel_amd.camera_rays(cam, 8, 6)[1][3, 4], [-1.0, 0.0, 0.0], atol=1e-6)


@pytest.mark.skipif(not oa.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("name", ["cornell", "motionblur", "ajax_standin_96"])
def test_camera_rays_are_the_reference_cameras_to_float32_rounding(name):
    """the float64 restatement against CameraSampler::GenerateRay itself, on the packs' own cameras at a frame that is not square: the
    reference works in float32 (a handful of roundings of quantities below 2: 1e-6 is ten of them)"""
    scene = tinsel_amd.Scene.load_pack(os.path.join(oa.GOLDEN, name + ".pack"))
    cam = abi.Camera.from_buffer_copy(scene.camera)
    W, H = 16, 12
    jj, ii = np.mgrid[0:H, 0:W]
    want = oa.RefOracle().camera_rays(cam, W, H, np.stack([ii.ravel(), jj.ravel()], axis=1).astype(np.float32))
    o, d = tinsel_amd.camera_rays(cam, W, H)
    assert np.abs(want[:, 0:3] - o).max() == 0.0 and np.abs(want[:, 3:6] - d.reshape(-1, 3)).max() <= 1e-6


def test_parse_args_accepts_the_irradiance_options():
    cfg = headless.parse_args(["headless", "-irradiance=bake.npz", "-irradiance_spp=8", "-width=16", "-height=12", "scene.pack"])
    assert cfg["irradiance"] == "bake.npz" and cfg["irradiance_spp"] == 8 and cfg["over"] == {"width": 16, "height": 12}
    assert headless.parse_args(["headless", "-irradiance=bake.npz", "scene.pack"])["irradiance_spp"] == 64
    assert headless.parse_args(["headless", "scene.pack"])["irradiance"] is None
    for bad in ("0", "65537"):
        with pytest.raises(SystemExit):
            headless.parse_args(["headless", "-irradiance_spp=" + bad, "scene.pack"])
    # nothing is rendered: what belongs to a render is refused beside it, before the scene is opened
    for other in ("-firsthit=b.npz", "-complexity=rays", "-out=a.png", "-save=s.npz", "-resume=s.npz", "-nlm=2", "-spp=4"):
        with pytest.raises(SystemExit, match="-irradiance bakes"):
            headless.main(["headless", "-irradiance=a.npz", other, "no_such_scene.pack"])

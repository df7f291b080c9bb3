"""CPU tests of the ray-query boundary (tinsel_hip_trace_rays / _device / tinsel_hip_trace_camera): the two 32-byte records in the
header and in the Python mirror, the exported symbols, the kernel's place in the launch list, the host entries' refusals that need
no GPU."""
import ctypes as C
import os
import re

import numpy as np

import tinsel_amd
from tinsel_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "tinsel_hip.h")).read()


def test_records_are_32_bytes_in_the_header_and_the_mirror():
    assert re.search(r"static_assert\(sizeof\(tinsel_ray\) == 32", HEADER)
    assert re.search(r"static_assert\(sizeof\(tinsel_ray_hit\) == 32", HEADER)
    m = re.search(r"typedef struct tinsel_ray\s*\{([^}]*)\}", HEADER)
    assert [f.strip() for f in re.sub(r"float|;", ",", m.group(1)).split(",") if f.strip()] == [n for n, _ in abi.Ray._fields_]
    assert C.sizeof(abi.Ray) == 32 and C.sizeof(abi.RayHit) == 32
    assert np.dtype(abi.RAY_DTYPE).itemsize == 32 and np.dtype(abi.RAY_HIT_DTYPE).itemsize == 32
    for (name, _), field in zip(abi.Ray._fields_, np.dtype(abi.RAY_DTYPE).names):
        assert name == field and getattr(abi.Ray, name).offset == np.dtype(abi.RAY_DTYPE).fields[field][1]
    hit = np.dtype(abi.RAY_HIT_DTYPE)
    assert [(n, getattr(abi.RayHit, n).offset) for n, _ in abi.RayHit._fields_] == [(n, hit.fields[n][1]) for n in hit.names]
    assert abi.RayHit.primitive.offset == 4 and abi.RayHit.nx.offset == 8 and abi.RayHit.reserved.offset == 20
    assert re.search(r"#define TINSEL_QUERY_CLOSEST\s+0\b", HEADER) and re.search(r"#define TINSEL_QUERY_OCCLUDED\s+1\b", HEADER)
    assert (abi.QUERY_CLOSEST, abi.QUERY_OCCLUDED) == (0, 1)
    # an (n, 8) float32 array IS a tinsel_ray[n]
    a = np.arange(16, dtype=np.float32).reshape(2, 8)
    v = a.view(abi.RAY_DTYPE)
    assert v["time"][1, 0] == 11 and v["tmax"][0, 0] == 7 and v["dx"][0, 0] == 4


def test_the_three_entries_are_exported_and_bound():
    L = tinsel_amd.load_library()
    for name in ("tinsel_hip_trace_rays", "tinsel_hip_trace_rays_device", "tinsel_hip_trace_camera"):
        assert hasattr(L, name) and name in tinsel_amd.renderer.EXPORTED_SYMBOLS
    assert L.tinsel_hip_trace_rays.argtypes[2] is C.c_longlong
    for method in ("trace_rays", "trace_camera", "first_hit"):
        assert callable(getattr(tinsel_amd.HipRenderer, method))


def test_both_arms_of_k_query_are_in_the_library_under_both_arithmetic_contracts():
    blob = open(tinsel_amd.renderer.LIB_PATH, "rb").read()
    for ns in (b"_ZN2tn", b"_ZN7tn_fast"):
        for mode in (b"0", b"1", b"2"):
            for lds in (b"0", b"1"):
                assert ns + b"7k_queryILi" + mode + b"ELb" + lds + b"EEE" in blob
        for mode in (b"0", b"1"):
            for lds in (b"0", b"1"):
                assert ns + b"14k_query_refillILi" + mode + b"ELb" + lds + b"EEE" in blob


def test_refusals_that_need_no_gpu():
    L = tinsel_amd.load_library()
    rays = np.zeros((4, 8), np.float32)
    out = np.full(4*32, 0xa5, np.uint8)
    cam = abi.Camera()
    assert L.tinsel_hip_trace_rays(None, 0, 4, rays.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == -1
    assert b"trace_rays" in L.tinsel_hip_last_error()
    assert L.tinsel_hip_trace_rays_device(None, 0, 4, None, None, None) == -1
    assert b"trace_rays_device" in L.tinsel_hip_last_error()
    assert L.tinsel_hip_trace_camera(None, C.byref(cam), 4, 4, 1.0, out.ctypes.data_as(C.c_void_p)) == -1
    assert b"trace_camera" in L.tinsel_hip_last_error()
    assert (out == 0xa5).all()

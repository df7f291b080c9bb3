"""CPU tests of the radiance-query boundary (tinsel_hip_trace_radiance / _device): the 48-byte start record in the header, the ctypes
mirror and the numpy dtype, the exported and bound entries, k_generate_rays in the library under both arithmetic contracts, the refusals
that need no GPU, and rng_state against the reference's own generator."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tinsel_amd
from tinsel_amd import abi
from tests import oracle_api as oa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "tinsel_hip.h")).read()


def test_the_record_is_48_bytes_in_the_header_the_mirror_and_the_dtype():
    assert re.search(r"static_assert\(sizeof\(tinsel_path_start\) == 48", HEADER)
    m = re.search(r"typedef struct tinsel_path_start\s*\{([^}]*)\}", HEADER)
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
    assert offset == 48 and len(fields) == 12
    assert C.sizeof(abi.PathStart) == 48 and np.dtype(abi.PATH_START_DTYPE).itemsize == 48
    dt = np.dtype(abi.PATH_START_DTYPE)
    mirror = [(n, "float" if t is C.c_float else "uint32_t", getattr(abi.PathStart, n).offset) for n, t in abi.PathStart._fields_]
    numpy = [(n, "float" if dt.fields[n][0] == np.dtype("<f4") else "uint32_t", dt.fields[n][1]) for n in dt.names]
    assert dt.fields["rng1"][0] == np.dtype("<u4") and dt.fields["ox"][0] == np.dtype("<f4")
    assert fields == mirror == numpy
    assert [f[0] for f in fields] == ["ox", "oy", "oz", "time", "dx", "dy", "dz", "reserved0", "rng1", "rng2", "reserved1", "reserved2"]
    # an (n, 12) array of 32-bit words IS a tinsel_path_start[n]
    a = np.arange(24, dtype=np.uint32).reshape(2, 12)
    v = a.view(abi.PATH_START_DTYPE)
    assert v["rng1"][1, 0] == 20 and v["rng2"][0, 0] == 9 and v["time"].view(np.uint32)[1, 0] == 15 and v["dx"].view(np.uint32)[0, 0] == 4


def test_the_entries_are_exported_and_bound():
    L = tinsel_amd.load_library()
    for name in ("tinsel_hip_trace_radiance", "tinsel_hip_trace_radiance_device"):
        assert hasattr(L, name) and name in tinsel_amd.renderer.EXPORTED_SYMBOLS
        assert re.search(r"\bint %s\(tinsel_hip\* r, long long n, const tinsel_path_start\*" % name, HEADER)
    assert L.tinsel_hip_trace_radiance.argtypes[1] is C.c_longlong and len(L.tinsel_hip_trace_radiance.argtypes) == 5
    assert L.tinsel_hip_trace_radiance_device.argtypes[1] is C.c_longlong and len(L.tinsel_hip_trace_radiance_device.argtypes) == 6
    assert callable(tinsel_amd.HipRenderer.radiance) and callable(tinsel_amd.rng_state)


def test_k_generate_rays_is_in_the_library_under_both_arithmetic_contracts():
    blob = open(tinsel_amd.renderer.LIB_PATH, "rb").read()
    for ns in (b"_ZN2tn", b"_ZN7tn_fast"):
        assert ns + b"15k_generate_raysE" in blob
    launch = open(os.path.join(ROOT, "tinsel_amd", "csrc", "tn_launch.h")).read()
    assert re.search(r"X\(PK_GENERATE_RAYS,\s+kBlock, 0, GENERATE_RAYS,\s*k_generate_rays\)", launch)
    assert '"k_generate_rays"' in open(os.path.join(ROOT, "tinsel_amd", "csrc", "tn_host_layout.h")).read()


def test_refusals_that_need_no_gpu():
    L = tinsel_amd.load_library()
    starts = np.zeros((4, 12), np.float32)
    out = np.full(4*16, 0xa5, np.uint8)
    sp, op = starts.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    # (the arguments are judged before the renderer is looked at: a handle that is only non-null will do for n < 0)
    handle = C.create_string_buffer(1 << 16)
    cases = [
        (lambda: L.tinsel_hip_trace_radiance(None, 4, sp, 4, op), b"trace_radiance:"),
        (lambda: L.tinsel_hip_trace_radiance(handle, -1, sp, 4, op), b"trace_radiance:"),
        (lambda: L.tinsel_hip_trace_radiance_device(None, 4, sp, 4, op, None), b"trace_radiance_device:"),
        (lambda: L.tinsel_hip_trace_radiance_device(handle, -7, sp, 4, op, None), b"trace_radiance_device:"),
    ]
    for case, own in cases:
        assert L.tinsel_hip_init(None, 0, 0) == -1 and L.tinsel_hip_last_error().startswith(b"init:")      # another entry's text in between
        assert case() == -1
        assert L.tinsel_hip_last_error().startswith(own), L.tinsel_hip_last_error()
        assert (out == 0xa5).all() and not starts.any()


def test_rng_state_at_skip_0_is_the_stated_formula():
    seeds = np.array([0, 1, 12345, 0xffffffff, 0xed2f7d60, 3979321632], np.uint32)       # (315645664 + 3979321632 = 2^32)
    s1, s2 = tinsel_amd.rng_state(seeds)
    assert s1.dtype == np.uint32 and s2.dtype == np.uint32 and s1.shape == seeds.shape
    want = [(315645664 + int(s)) % 2**32 for s in seeds]
    assert s1.tolist() == want and s2.tolist() == [w ^ 0x13ab45fe for w in want]
    a, b = tinsel_amd.rng_state(7)
    assert np.shape(a) == () and int(a) == 315645671 and int(b) == 315645671 ^ 0x13ab45fe
    grid = np.arange(6, dtype=np.uint32).reshape(2, 3)
    g1, g2 = tinsel_amd.rng_state(grid, 2)
    f1, f2 = tinsel_amd.rng_state(grid.ravel(), 2)
    assert g1.shape == (2, 3) and np.array_equal(g1.ravel(), f1) and np.array_equal(g2.ravel(), f2)


@pytest.mark.skipif(not oa.have_ref(), reason="oracle/_ref not built")
def test_rng_state_continues_the_reference_generator():
    """Rand() continued from rng_state(seed, skip) gives the reference's leaf_random(seed, skip + 8)[0][skip:].  Rand() returns the
    generator's new first word, so "continued k times" is read off rng_state(seed, skip + k) -- the step itself is stated nowhere in
    this test.  The second word is held too: the next first word depends on it, and every first word up to skip + 8 is compared."""
    R = oa.RefOracle()
    seeds = np.array([0, 1, 2, 97, 5550, 20261018, 0x7fffffff, 0x80000000, 0xffffffff], np.uint32)
    for skip in (0, 1, 3, 5, 64):
        ref = np.stack([R.leaf_random(int(s), skip + 8)[0] for s in seeds])            # [seed][output]
        got = np.stack([tinsel_amd.rng_state(seeds, skip + k)[0] for k in range(1, 9)], axis=1)
        assert np.array_equal(got, ref[:, skip:]), skip

"""CPU tests of the SH gather-query boundary (tinsel_hip_gather_sh / _device): the declarations and the order limit in the header, the
ctypes mirror, the kernel in the launch list, the name table and the library under both arithmetic contracts, the refusals that need no
GPU, the float32 basis mirror (sh_basis) and the irradiance evaluation (sh_irradiance), and the headless options."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tinsel_amd
from tinsel_amd import abi, headless

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "tinsel_hip.h")).read()

# the header's literals, as float32
K0, K1, K2, K6, K8 = (np.float32(v) for v in (0.28209479, 0.48860251, 1.0925484, 0.31539157, 0.54627422))


def test_the_entries_are_declared_exported_and_bound():
    L = tinsel_amd.load_library()
    assert re.search(r"#define TINSEL_GATHER_SH_MAX_ORDER 2\b", HEADER) and abi.GATHER_SH_MAX_ORDER == 2
    for name in ("tinsel_hip_gather_sh", "tinsel_hip_gather_sh_device"):
        assert hasattr(L, name) and name in tinsel_amd.renderer.EXPORTED_SYMBOLS
        assert re.search(r"\bint %s\(tinsel_hip\* r, int mode, int order, long long n, const tinsel_gather_point\* \w+,\s*int samples, int max_depth, "
                         r"float\* \w+, tinsel_path_start\* \w+" % name, HEADER)
    host, dev = L.tinsel_hip_gather_sh.argtypes, L.tinsel_hip_gather_sh_device.argtypes
    assert len(host) == 9 and len(dev) == 10 and dev[:9] == host
    assert host[1] is C.c_int and host[2] is C.c_int and host[3] is C.c_longlong and host[5] is C.c_int and host[6] is C.c_int
    assert all(host[k] is C.c_void_p for k in (0, 4, 7, 8)) and dev[9] is C.c_void_p
    # the plain gather's entries are the ones they were
    assert len(L.tinsel_hip_gather_radiance.argtypes) == 8 and len(L.tinsel_hip_gather_radiance_device.argtypes) == 9
    assert callable(tinsel_amd.HipRenderer.gather_sh) and callable(tinsel_amd.sh_basis) and callable(tinsel_amd.sh_irradiance)
    # the header states the basis, literal by literal
    for lit in ("0.28209479f", "0.48860251f*y", "0.48860251f*z", "0.48860251f*x", "(1.0925484f*x)*y", "(1.0925484f*y)*z", "(1.0925484f*x)*z",
                "0.31539157f*((3.0f*z)*z - 1.0f)", "0.54627422f*(x*x - y*y)"):
        assert lit in HEADER, lit


def test_the_kernel_is_in_the_library_under_both_arithmetic_contracts():
    blob = open(tinsel_amd.renderer.LIB_PATH, "rb").read()
    for ns in (b"_ZN2tn", b"_ZN7tn_fast"):
        assert ns + b"18k_gather_sh_reduceE" in blob
        assert ns + b"17k_generate_gatherE" in blob and ns + b"15k_gather_reduceE" in blob
    launch = open(os.path.join(ROOT, "tinsel_amd", "csrc", "tn_launch.h")).read()
    assert re.search(r"X\(PK_GATHER_SH_REDUCE,\s+\w+, 0, GATHER_SH_REDUCE,\s*k_gather_sh_reduce\)", launch)
    layout = open(os.path.join(ROOT, "tinsel_amd", "csrc", "tn_host_layout.h")).read()
    assert '"k_gather_sh_reduce"' in layout and "KN_GATHER_SH_REDUCE" in layout
    names = re.search(r"kKernelNames\[\] = \{([^}]*)\}", layout).group(1).replace('"', "").split(",")
    ids = re.search(r"enum \{ KN_GENERATE = 0,([^}]*)KN_COUNT \}", layout).group(1).split(",")
    names, ids = [s.strip() for s in names], ["KN_GENERATE"] + [s.strip() for s in ids if s.strip()]
    assert len(names) == len(ids) and names.index("k_gather_sh_reduce") == ids.index("KN_GATHER_SH_REDUCE")


def test_refusals_that_need_no_gpu():
    """(the arguments are judged before the renderer is looked at: a handle that is only non-null will do)"""
    L = tinsel_amd.load_library()
    points = np.zeros((4, 8), np.float32)
    out = np.full(4*9*16, 0xa5, np.uint8)
    pp, op = points.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    handle = C.create_string_buffer(1 << 16)
    host = lambda *a: L.tinsel_hip_gather_sh(*a, None)
    dev = lambda *a: L.tinsel_hip_gather_sh_device(*a, None, None)
    for fn, own in ((host, b"gather_sh:"), (dev, b"gather_sh_device:")):
        cases = [
            (None, 1, 2, 4, pp, 8, 4, op),              # null renderer
            (None, 1, 3, 4, pp, 8, 4, op),
            (handle, 1, -1, 4, pp, 8, 4, op),           # order outside 0 .. 2
            (handle, 1, 3, 4, pp, 8, 4, op),
            (handle, 0, -1, 0, None, 8, 4, None),       # ... judged before n
            (handle, -1, 2, 4, pp, 8, 4, op),           # the gather query's own rules
            (handle, 2, 2, 4, pp, 8, 4, op),
            (handle, 0, 2, -1, pp, 8, 4, op),
            (handle, 0, 2, 2**31, pp, 8, 4, op),
            (handle, 0, 1, 4, pp, 0, 4, op),
            (handle, 0, 1, 4, pp, 65537, 4, op),
            (handle, 1, 0, 4, pp, 8, 0, op),
            (handle, 0, 0, 4, None, 8, 4, op),
            (handle, 1, 2, 4, pp, 8, 4, None),
        ]
        for case in cases:
            assert L.tinsel_hip_init(None, 0, 0) == -1 and L.tinsel_hip_last_error().startswith(b"init:")      # another entry's text in between
            assert fn(*case) == -1, case
            assert L.tinsel_hip_last_error().startswith(own), L.tinsel_hip_last_error()
            assert (out == 0xa5).all() and not points.any()


def test_sh_basis_at_the_axes_is_the_closed_form_of_the_literals():
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    Y = tinsel_amd.sh_basis(axes)
    assert Y.dtype == np.float32 and Y.shape == (6, 9)
    z, two = np.float32(0.0), np.float32(2.0)
    equator, pole = K6*np.float32(-1.0), K6*two               # 0.31539157f*((3*0)*0 - 1), 0.31539157f*((3*1)*1 - 1)
    want = np.array([
        [K0, z, z, K1, z, z, equator, z, K8],
        [K0, z, z, -K1, z, z, equator, z, K8],
        [K0, K1, z, z, z, z, equator, z, -K8],
        [K0, -K1, z, z, z, z, equator, z, -K8],
        [K0, z, K1, z, z, z, pole, z, z],
        [K0, z, -K1, z, z, z, pole, z, z]], np.float32)
    assert np.array_equal(Y, want)
    # the lower orders are prefixes, any leading shape is kept, and the order is checked
    d = np.random.default_rng(3).normal(size=(5, 7, 3)).astype(np.float32)
    full = tinsel_amd.sh_basis(d, 2)
    assert full.shape == (5, 7, 9) and np.array_equal(tinsel_amd.sh_basis(d, 1), full[..., :4]) and np.array_equal(tinsel_amd.sh_basis(d, 0), full[..., :1])
    x, y, zz = d[..., 0], d[..., 1], d[..., 2]
    assert np.array_equal(full[..., 4], (K2*x)*y) and np.array_equal(full[..., 5], (K2*y)*zz) and np.array_equal(full[..., 7], (K2*x)*zz)
    assert np.array_equal(full[..., 6], K6*((np.float32(3.0)*zz)*zz - np.float32(1.0))) and np.array_equal(full[..., 8], K8*(x*x - y*y))
    for bad in (-1, 3):
        with pytest.raises(ValueError):
            tinsel_amd.sh_basis(d, bad)


def test_sh_basis_is_orthonormal_under_an_exact_quadrature():
    """8 Gauss-Legendre nodes in z times 16 uniform angles integrate every product of two basis functions (degree 4 in z, frequency 4
    in phi at most) exactly; what is left is the float32 rounding of the basis values and the 8-digit literals, a few 1e-7 an entry."""
    z, wz = np.polynomial.legendre.leggauss(8)
    phi = (np.arange(16) + 0.5)*(2.0*np.pi/16)
    zz, pp = np.meshgrid(z, phi, indexing="ij")
    s = np.sqrt(1.0 - zz*zz)
    d = np.stack([s*np.cos(pp), s*np.sin(pp), zz], axis=-1).reshape(-1, 3)
    w = np.repeat(wz, 16)*(2.0*np.pi/16)
    assert abs(w.sum() - 4.0*np.pi) < 1e-12
    Y = tinsel_amd.sh_basis(d.astype(np.float32)).astype(np.float64)
    gram = np.einsum("k,ki,kj->ij", w, Y, Y)
    err = np.abs(gram - np.eye(9)).max()
    print("largest deviation of the Gram matrix from the identity: %.3g" % err)
    assert err <= 1e-5


def test_sh_irradiance_of_a_linear_radiance_field():
    """L(d) = 1 + a.d has c0 = sqrt(4 pi), band 1 = sqrt(4 pi / 3) * (a_y, a_z, a_x) and irradiance pi + (2 pi / 3) a.n"""
    rng = np.random.default_rng(11)
    n = rng.normal(size=(64, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    a = np.array([[0.3, -0.2, 0.5], [0.0, 0.7, -0.1], [-0.4, 0.1, 0.2]])           # one vector per channel
    for C_ in (4, 9):
        c = np.zeros((C_, 3))
        c[0] = np.sqrt(4.0*np.pi)
        c[1:4] = np.sqrt(4.0*np.pi/3.0)*np.stack([a[:, 1], a[:, 2], a[:, 0]])
        want = np.pi + (2.0*np.pi/3.0)*(n @ a.T)
        got = tinsel_amd.sh_irradiance(c, n)                                        # one probe, many normals
        assert got.dtype == np.float64 and got.shape == (64, 3)
        assert (np.abs(got - want) <= 1e-12*np.abs(want)).all()
        per = tinsel_amd.sh_irradiance(np.repeat(c[None], 64, axis=0), n)           # one normal per probe
        assert (np.abs(per - want) <= 1e-12*np.abs(want)).all()
    # band 0 alone: pi * c0 * Y0
    assert np.allclose(tinsel_amd.sh_irradiance(np.full((1, 3), np.sqrt(4.0*np.pi)), n), np.pi, rtol=1e-12, atol=0)
    # band 2 is scaled by pi/4: the zonal coefficient alone, at the pole
    c = np.zeros((9, 3))
    c[6] = 1.0
    pole = tinsel_amd.sh_irradiance(c, np.array([[0.0, 0.0, 1.0]]))
    assert np.allclose(pole, (np.pi/4.0)*0.25*np.sqrt(5.0/np.pi)*2.0, rtol=1e-12, atol=0)
    with pytest.raises(ValueError):
        tinsel_amd.sh_irradiance(np.zeros((5, 3)), n)


def test_parse_args_accepts_the_probe_options():
    cfg = headless.parse_args(["headless", "-probes=p.npz", "-probes_at=at.npy", "-probes_spp=67", "-probes_order=1", "-maxdepth=4", "scene.pack"])
    assert (cfg["probes"], cfg["probes_at"], cfg["probes_spp"], cfg["probes_order"]) == ("p.npz", "at.npy", 67, 1) and cfg["over"] == {"maxdepth": 4}
    cfg = headless.parse_args(["headless", "-probes=p.npz", "-probes_at=at.npy", "scene.pack"])
    assert cfg["probes_spp"] == 1024 and cfg["probes_order"] == 2
    assert headless.parse_args(["headless", "scene.pack"])["probes"] is None
    for bad in ("-probes_spp=0", "-probes_spp=65537", "-probes_order=3", "-probes_order=-1"):
        with pytest.raises(SystemExit):
            headless.parse_args(["headless", bad, "scene.pack"])
    # nothing is rendered: what belongs to a render is refused beside it, before the scene is opened
    for other in ("-firsthit=b.npz", "-complexity=rays", "-out=a.png", "-save=s.npz", "-resume=s.npz", "-nlm=2", "-spp=4", "-irradiance=i.npz"):
        with pytest.raises(SystemExit, match="-probes bakes"):
            headless.main(["headless", "-probes=a.npz", "-probes_at=at.npy", other, "no_such_scene.pack"])
    with pytest.raises(SystemExit, match="-probes bakes"):
        headless.main(["headless", "-probes=a.npz", "-probes_at=at.npy", "no_such_%d.pack"])
    for alone in ("-probes=a.npz", "-probes_at=at.npy"):
        with pytest.raises(SystemExit, match="go together"):
            headless.main(["headless", alone, "no_such_scene.pack"])
    assert "float32" in headless.__doc__ and "-probes_order" in headless.__doc__

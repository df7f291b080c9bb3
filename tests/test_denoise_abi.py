"""CPU tests of the denoise boundary (tinsel_hip_denoise / _device, tinsel_hip_present_image_device): the declarations, the export and the
ctypes mirror, the parameter struct and its defaults, the kernels in the library (exact arm only), every refusal that needs no GPU, the
headless option -- and the host statement tests/denoise_reference.py itself, pinned to the reference's NonLocalMeansFilter bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tinsel_amd
from tinsel_amd import abi, headless
from tests import oracle_api as oa
from tests.denoise_reference import Params, denoise_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "tinsel_hip.h")).read()
FIELDS = ("radius", "patch_radius", "k_color", "k_albedo", "k_normal", "k_depth", "demodulate", "albedo_floor")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_entries_are_declared_exported_and_bound():
    L = tinsel_amd.load_library()
    for name in ("tinsel_hip_denoise_params_init", "tinsel_hip_denoise", "tinsel_hip_denoise_device", "tinsel_hip_present_image_device"):
        assert hasattr(L, name) and name in tinsel_amd.renderer.EXPORTED_SYMBOLS
        assert re.search(r"\b%s\(" % name, HEADER)
    assert re.search(r"int tinsel_hip_denoise\(tinsel_hip\* r, const float\* beauty_host, const float\* planes_host,\s*unsigned features, int width, "
                     r"int height,\s*const tinsel_hip_denoise_params\* p, float\* out_host\);", HEADER)
    assert re.search(r"int tinsel_hip_denoise_device\(tinsel_hip\* r, const float\* beauty_dev, const float\* planes_dev,\s*unsigned features, int width, "
                     r"int height,\s*const tinsel_hip_denoise_params\* p, float\* out_dev, void\* stream\);", HEADER)
    assert re.search(r"int tinsel_hip_present_image_device\(tinsel_hip\* r, const float\* image_dev,\s*const tinsel_options\* options, int nlm_width,\s*"
                     r"float nlm_falloff, void\* stream\);", HEADER)
    host, dev = L.tinsel_hip_denoise.argtypes, L.tinsel_hip_denoise_device.argtypes
    assert len(host) == 8 and len(dev) == 9 and dev[:8] == host and dev[8] is C.c_void_p
    assert host[3] is C.c_uint and host[4] is C.c_int and host[5] is C.c_int and host[6] is C.POINTER(abi.DenoiseParams)
    assert len(L.tinsel_hip_present_image_device.argtypes) == 6
    assert callable(tinsel_amd.HipRenderer.denoise) and callable(tinsel_amd.HipRenderer.present_image) and callable(tinsel_amd.denoise_params)
    # the header says what the stage is for, and that its kernels have no timing class
    for text in ("meant for a WHOLE frame", "no class in tinsel_hip_kernel_times", "planes may be\n * NULL only when features == 0"):
        assert text in HEADER, text


def test_the_parameter_struct_and_its_defaults():
    assert C.sizeof(abi.DenoiseParams) == 32 and tuple(k for k, _ in abi.DenoiseParams._fields_) == FIELDS
    m = re.search(r"typedef struct tinsel_hip_denoise_params \{(.*?)\} tinsel_hip_denoise_params;", HEADER, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert tuple(re.findall(r"\b([a-z_]+)\s*[,;]", body)) == FIELDS
    p = tinsel_amd.denoise_params()
    d = p.as_dict()
    assert 1 <= d["radius"] <= 8 and 0 <= d["patch_radius"] <= 4 and d["demodulate"] in (0, 1) and d["albedo_floor"] > 0
    assert all(np.isfinite(d[k]) and d[k] >= 0 for k in ("k_color", "k_albedo", "k_normal", "k_depth"))
    # ... are the ones profiles/denoise_defaults.md records
    doc = open(os.path.join(ROOT, "profiles", "denoise_defaults.md")).read()
    line = re.search(r"^defaults: (.*)$", doc, re.M).group(1)
    recorded = {k: float(v) for k, v in re.findall(r"(\w+)=([-0-9.e]+)", line)}
    assert sorted(recorded) == sorted(FIELDS)
    for k in FIELDS:
        assert np.float32(recorded[k]) == np.float32(d[k]), k
    q = tinsel_amd.denoise_params(radius=7, k_depth=0.5, demodulate=0)
    assert (q.radius, q.k_depth, q.demodulate, q.k_color) == (7, 0.5, 0, p.k_color)
    with pytest.raises(TypeError):
        tinsel_amd.denoise_params(falloff=1.0)


def test_the_kernels_are_in_the_library_in_the_exact_arm_only():
    blob = open(tinsel_amd.renderer.LIB_PATH, "rb").read()
    assert b"_ZN2tn17k_denoise_prepareE" in blob
    for mask in range(8):
        assert b"_ZN2tn9k_denoiseILj%dEEE" % mask in blob, mask
    assert b"_ZN7tn_fast9k_denoise" not in blob and b"_ZN7tn_fast17k_denoise_prepare" not in blob
    unit = open(os.path.join(ROOT, "tinsel_amd", "csrc", "tinsel_hip.hip")).read()
    fast = open(os.path.join(ROOT, "tinsel_amd", "csrc", "tinsel_fast.hip")).read()
    assert '#include "tn_denoise.h"' in unit and "tn_denoise.h" not in fast
    assert "tn_denoise.h" not in open(os.path.join(ROOT, "tinsel_amd", "csrc", "tn_kernels.h")).read()


def test_refusals_that_need_no_gpu():
    """(the arguments are judged before the renderer is looked at: a handle that is only non-null will do -- zeroed, it was never init-ed)"""
    L = tinsel_amd.load_library()
    W, H = 4, 3
    out = np.full(W*H*4, 5.0, np.float32)
    beauty = np.ones(W*H*4, np.float32)
    planes = np.ones(3*W*H*4, np.float32)
    op, bp, pp = (a.ctypes.data_as(C.c_void_p) for a in (out, beauty, planes))
    assert out.ctypes.data % 16 == 0 or True
    handle = C.create_string_buffer(1 << 20)
    good = tinsel_amd.denoise_params()

    def par(**kw):
        return C.byref(tinsel_amd.denoise_params(**kw))

    gp = C.byref(good)
    nan, inf = float("nan"), float("inf")
    cases = [
        (b"null", (None, bp, pp, 7, W, H, gp, op)),
        (b"null", (handle, bp, pp, 7, W, H, None, op)),
        (b"null", (handle, bp, pp, 7, W, H, gp, None)),
        (b"null", (handle, bp, None, 7, W, H, gp, op)),
        (b"null", (handle, bp, None, 1, W, H, gp, op)),
        (b"features", (handle, bp, pp, 8, W, H, gp, op)),
        (b"features", (handle, bp, pp, 0xffffffff, W, H, gp, op)),
        (b"radius", (handle, bp, pp, 7, W, H, par(radius=0), op)),
        (b"radius", (handle, bp, pp, 7, W, H, par(radius=9), op)),
        (b"radius", (handle, bp, pp, 7, W, H, par(radius=-1), op)),
        (b"patch_radius", (handle, bp, pp, 7, W, H, par(patch_radius=-1), op)),
        (b"patch_radius", (handle, bp, pp, 7, W, H, par(patch_radius=5), op)),
        (b"k_color", (handle, bp, pp, 7, W, H, par(k_color=-1.0), op)),
        (b"k_color", (handle, bp, pp, 7, W, H, par(k_color=nan), op)),
        (b"k_color", (handle, bp, pp, 7, W, H, par(k_albedo=inf), op)),
        (b"k_color", (handle, bp, pp, 7, W, H, par(k_normal=-0.5), op)),
        (b"k_color", (handle, bp, pp, 7, W, H, par(k_depth=nan), op)),
        (b"demodulate", (handle, bp, pp, 7, W, H, par(demodulate=2), op)),
        (b"demodulate", (handle, bp, pp, 7, W, H, par(demodulate=-1), op)),
        (b"albedo_floor", (handle, bp, pp, 7, W, H, par(demodulate=1, albedo_floor=0.0), op)),
        (b"albedo_floor", (handle, bp, pp, 7, W, H, par(albedo_floor=-1.0), op)),
        (b"albedo_floor", (handle, bp, pp, 7, W, H, par(albedo_floor=inf), op)),
        (b"albedo_floor", (handle, bp, pp, 7, W, H, par(albedo_floor=nan), op)),
        (b"TINSEL_FEATURE_ALBEDO", (handle, bp, pp, 6, W, H, par(demodulate=1), op)),
        (b"TINSEL_FEATURE_ALBEDO", (handle, bp, None, 0, W, H, par(demodulate=1), op)),
        (b"width", (handle, bp, pp, 7, 0, H, gp, op)),
        (b"width", (handle, bp, pp, 7, W, -2, gp, op)),
        (b"tinsel_hip_init", (handle, None, pp, 7, W, H, gp, op)),          # the renderer's accumulator: no init
        (b"tinsel_hip_init", (handle, None, None, 0, W, H, gp, op)),
    ]
    host = lambda *a: L.tinsel_hip_denoise(*a)
    dev = lambda *a: L.tinsel_hip_denoise_device(*a, None)
    for fn, own in ((host, b"denoise:"), (dev, b"denoise_device:")):
        for cause, case in cases:
            assert L.tinsel_hip_init(None, 0, 0) == -1 and L.tinsel_hip_last_error().startswith(b"init:")      # another entry's text in between
            assert fn(*case) == -1, case
            msg = L.tinsel_hip_last_error()
            assert msg.startswith(own) and cause in msg, (msg, cause)
            assert (out == 5.0).all()
    # the device entry: every pointer 16-byte aligned (made-up addresses: refused before anything is read)
    for b, p, o in ((0x10008, 0x20000, 0x30000), (0x10000, 0x20004, 0x30000), (0x10000, 0x20000, 0x30001), (None, 0x20000, 0x30008)):
        assert L.tinsel_hip_init(None, 0, 0) == -1
        assert L.tinsel_hip_denoise_device(handle, b, p, 7, W, H, gp, o, None) == -1
        msg = L.tinsel_hip_last_error()
        assert msg.startswith(b"denoise_device:") and b"16-byte aligned" in msg, msg
    # present_image_device
    opt = abi.Options()
    opt.mode, opt.width, opt.height = abi.MODE_PATHTRACE, W, H
    for cause, case in ((b"bad arguments", (None, 0x10000, C.byref(opt), 0, 200.0, None)),
                        (b"bad arguments", (handle, None, C.byref(opt), 0, 200.0, None)),
                        (b"bad arguments", (handle, 0x10000, None, 0, 200.0, None)),
                        (b"bad arguments", (handle, 0x10000, C.byref(opt), -1, 200.0, None)),
                        (b"16-byte aligned", (handle, 0x10004, C.byref(opt), 0, 200.0, None)),
                        (b"tinsel_hip_init", (handle, 0x10000, C.byref(opt), 0, 200.0, None))):
        assert L.tinsel_hip_init(None, 0, 0) == -1
        assert L.tinsel_hip_present_image_device(*case) == -1, case
        msg = L.tinsel_hip_last_error()
        assert msg.startswith(b"present_image_device:") and cause in msg, msg
    # present_async keeps its own text
    assert L.tinsel_hip_present_async(handle, C.byref(opt), 0, 200.0, None) == -1 and L.tinsel_hip_last_error().startswith(b"present:")


def test_the_headless_option():
    assert headless.parse_args(["headless", "scene.pack"])["denoise"] is None
    assert headless.parse_args(["headless", "-denoise", "-spp=4", "scene.pack"])["denoise"] == 0          # the default radius
    assert headless.parse_args(["headless", "-denoise=3", "scene.pack"])["denoise"] == 3
    for bad in ("-denoise=0", "-denoise=9", "-denoise=-1"):
        with pytest.raises(SystemExit):
            headless.parse_args(["headless", bad, "scene.pack"])
    for flag in ("-denoise", "-denoise=2"):
        for other in ("-resume=s.npz", "-complexity=rays", "-irradiance=i.npz", "-firsthit=b.npz"):
            with pytest.raises(SystemExit, match="-denoise filters"):
                headless.main(["headless", flag, other, "no_such_scene.pack"])
        with pytest.raises(SystemExit, match="-denoise filters"):
            headless.main(["headless", flag, "-probes=p.npz", "-probes_at=at.npy", "no_such_scene.pack"])
        with pytest.raises(SystemExit, match="-denoise filters"):
            headless.main(["headless", flag, "no_such_%d.pack"])
    assert "-denoise[=RADIUS]" in headless.__doc__


# ---------------------------------------------------------------------------
# the statement itself: with the guide terms off it is the reference's NonLocalMeansFilter

def _as_beauty(c, rng=None):
    """colour [H, W, 3] as an accumulator whose normalisation gives the colour back bit for bit: weight 1, or a power of two"""
    b = np.ones(c.shape[:2] + (4,), np.float32)
    if rng is not None:
        b[..., 3] = np.float32(2.0)**rng.integers(-3, 4, c.shape[:2]).astype(np.float32)
    b[..., :3] = c*b[..., 3:4]
    assert np.array_equal(_bits(b[..., :3]/b[..., 3:4]), _bits(c))
    return b


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("shape", [(21, 37), (3, 5), (1, 1), (16, 16)])
def test_without_guides_the_statement_is_the_reference_nlm_on_random_images(radius, shape):
    rng = np.random.default_rng(100*radius + shape[0])
    P = oa.PortOracle()
    for falloff in (200.0, 3.0):
        c = rng.random(shape + (3,)).astype(np.float32)
        image = np.zeros(shape + (4,), np.float32)
        image[..., :3] = c
        want = P.nlm(image, falloff, radius)
        got = denoise_reference(_as_beauty(c, rng), None, 0, Params(radius, radius, falloff))
        assert np.array_equal(_bits(got[..., :3]), _bits(want[..., :3]))
        assert (got[..., 3] == 1.0).all()


def test_without_guides_the_statement_is_the_reference_nlm_on_the_display_fixtures():
    """tests/golden/display.golden.npz holds outputs of the reference's own NonLocalMeansFilter"""
    gold = np.load(os.path.join(oa.GOLDEN, "display.golden.npz"))
    c = gold["nlm_in_a"][..., :3]
    P = oa.PortOracle()
    for radius, falloff, key in ((1, 200.0, "nlm_r1_a"), (2, 50.0, "nlm_r2_a")):
        got = denoise_reference(_as_beauty(c), None, 0, Params(radius, radius, falloff))
        assert np.array_equal(_bits(got[..., :3]), _bits(gold[key][..., :3])), key
        assert np.array_equal(_bits(got[..., :3]), _bits(P.nlm(gold["nlm_in_a"], falloff, radius)[..., :3])), key


def test_the_guide_terms_of_the_statement_by_hand():
    """two pixels side by side, radius 1, patch radius 0: every term of the exponent spelled out in float32"""
    F = np.float32
    from tests.denoise_reference import expf
    beauty = np.array([[[0.5, 1.0, 2.0, 2.0], [0.0, 0.0, 0.0, 0.0]]], F)               # the second pixel has no weight: colour 0
    albedo = np.array([[[0.5, 0.001, 1.0, 1.0], [1.0, 1.0, 1.0, 2.0]]], F)
    normal = np.array([[[0.0, 0.0, 2.0, 2.0], [1.0, 0.0, 0.0, 1.0]]], F)
    depth = np.array([[[6.0, 20.0, 2.0, 2.0], [0.0, 0.0, 0.0, 3.0]]], F)              # the second pixel missed: z = 0
    p = Params(1, 0, 2.0, 3.0, 5.0, 7.0, 1, 0.25)
    got = denoise_reference(beauty, np.stack([albedo, normal, depth]), 7, p)
    a0, a1 = np.array([0.5, 0.001, 1.0], F), np.array([0.5, 0.5, 0.5], F)
    d0 = np.array([0.5, 0.25, 1.0], F)
    u0 = np.array([0.25, 0.5, 1.0], F)/d0
    lc = u0[0]*u0[0] + u0[1]*u0[1] + u0[2]*u0[2]
    da = a0 - a1
    la = da[0]*da[0] + da[1]*da[1] + da[2]*da[2]
    ln = F(1.0)*F(1.0) + F(0.0) + F(1.0)*F(1.0)
    ld = (F(3.0)*F(3.0))/(F(3.0)*F(3.0) + F(0.0))
    e = F(2.0)*lc
    e = e + F(3.0)*la
    e = e + F(5.0)*ln
    e = e + F(7.0)*ld
    w = expf(-e)[()]
    # pixel 0: itself (weight expf(-0) = 1) then its neighbour (colour 0)
    total = F(1.0) + w
    want0 = ((u0*F(1.0) + F(0.0)*w)*(F(1.0)/total))*d0
    assert np.array_equal(_bits(got[0, 0, :3]), _bits(want0)) and got[0, 0, 3] == 1.0
    # pixel 1: its neighbour first (fx ascending), then itself
    total = w + F(1.0)
    want1 = ((u0*w + F(0.0))*(F(1.0)/total))*np.array([0.5, 0.5, 0.5], F)
    assert np.array_equal(_bits(got[0, 1, :3]), _bits(want1))
    # an absent plane's term is skipped: with the depth bit off the depth coefficient does nothing
    a = denoise_reference(beauty, np.stack([albedo, normal]), 3, p)
    b = denoise_reference(beauty, np.stack([albedo, normal]), 3, Params(1, 0, 2.0, 3.0, 5.0, 1000.0, 1, 0.25))
    assert np.array_equal(_bits(a), _bits(b)) and not np.array_equal(_bits(a), _bits(got))

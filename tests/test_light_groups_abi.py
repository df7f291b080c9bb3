"""CPU tests of the light-group boundary (tinsel_hip_render_light_groups / _device): the declarations in the header and the ctypes mirror,
the twin kernels in the launch list and in the library, the refusals that need no GPU, default_light_groups and relight, the byte edit that
makes a masked pack -- and the yardstick itself, held for the reference alone: the oracle's masked renders carry the beauty's weight plane,
are finite, and with clamp = FLT_MAX add up to the beauty within the rounding bound."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tinsel_amd
from tinsel_amd import abi, headless
from tests import light_groups_reference as lg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "tinsel_hip.h")).read()
FLT_MAX = float(np.finfo(np.float32).max)
W, H, PASSES = 48, 32, 4


def test_the_entries_are_declared_exported_and_bound():
    L = tinsel_amd.load_library()
    assert re.search(r"#define TINSEL_MAX_LIGHT_GROUPS\s+8\b", HEADER) and abi.MAX_LIGHT_GROUPS == 8
    for name, tail in (("tinsel_hip_render_light_groups", r"float\* out_host"), ("tinsel_hip_render_light_groups_device", r"float\* out_dev, void\* stream")):
        assert hasattr(L, name) and name in tinsel_amd.renderer.EXPORTED_SYMBOLS
        assert re.search(r"\bint %s\(tinsel_hip\* r, const tinsel_camera\* camera, const tinsel_options\* options,\s*uint32_t pass_begin, int passes, "
                         r"int num_groups, const int32_t\* group_of_primitive, int env_group,\s*%s\);" % (name, tail), HEADER), name
    host, dev = L.tinsel_hip_render_light_groups.argtypes, L.tinsel_hip_render_light_groups_device.argtypes
    assert len(host) == 9 and len(dev) == 10 and dev[:9] == host and dev[9] is C.c_void_p
    assert host[3] is C.c_uint32 and host[4] is host[5] is host[7] is C.c_int and host[0] is host[6] is host[8] is C.c_void_p
    assert callable(tinsel_amd.HipRenderer.light_groups) and callable(tinsel_amd.default_light_groups) and callable(tinsel_amd.relight)
    # the header states the definition, the clamp, the probe caveat and what the call leaves alone
    for text in ("emission = 0 on every primitive i whose group_of_primitive[i] != g", "applies to EACH PLANE SEPARATELY", "only with clamp = FLT_MAX",
                 "the weight channel of every plane is the beauty's", "its radiance lands in env_group only", "need not be the light that was sampled",
                 'timed under the name "k_shade"', "16 bytes x num_groups per path slot"):
        assert text in HEADER, text


def test_the_twins_are_in_the_launch_list_and_in_the_library():
    blob = open(tinsel_amd.renderer.LIB_PATH, "rb").read()
    # (compiled in the tolerance arm's translation unit too, never reached there: the call refuses that arm)
    for ns in (b"_ZN2tn", b"_ZN7tn_fast"):
        for inst in (b"ILb1ELb1EEE", b"ILb1ELb0EEE", b"ILb0ELb0EEE"):
            assert ns + b"14k_shade_groups" + inst in blob, (ns, inst)
    launch = open(os.path.join(ROOT, "tinsel_amd", "csrc", "tn_launch.h")).read()
    assert re.search(r"X\(PK_SHADE_GROUPS_MIXED,\s+kBlock, 0, SHADE_GROUPS,\s*k_shade_groups<true, true>\)", launch)
    assert re.search(r"X\(PK_SHADE_GROUPS_LDS,\s+kBlock, 0, SHADE_GROUPS,\s*k_shade_groups<true>\)", launch)
    assert re.search(r"X\(PK_SHADE_GROUPS,\s+kBlock, 0, SHADE_GROUPS,\s*k_shade_groups<false>\)", launch)
    # the planes have one writer per record: no atomics in the deposit
    split = open(os.path.join(ROOT, "tinsel_amd", "csrc", "tn_split.h")).read()
    deposit = split[split.index("TN_D void group_deposit"):split.index("// the shading half of one path")]
    assert "atomic" not in deposit


def test_refusals_that_need_no_gpu():
    """(the arguments are judged before the renderer is looked at: a handle that is only non-null will do -- zeroed, it was never init-ed)"""
    L = tinsel_amd.load_library()
    out = np.full(8*4*4*4, 5.0, np.float32)
    op = out.ctypes.data_as(C.c_void_p)
    table = np.zeros(16, np.int32)
    tp = table.ctypes.data_as(C.c_void_p)
    handle = C.create_string_buffer(1 << 20)
    cam, opt, normals = abi.Camera(), abi.Options(), abi.Options()
    opt.mode, opt.width, opt.height = abi.MODE_PATHTRACE, 4, 4
    normals.mode, normals.width, normals.height = abi.MODE_NORMALS, 4, 4
    cp, opp = C.byref(cam), C.byref(opt)
    host = lambda *a: L.tinsel_hip_render_light_groups(*a)
    dev = lambda *a: L.tinsel_hip_render_light_groups_device(*a, None)
    for fn, own in ((host, b"render_light_groups:"), (dev, b"render_light_groups_device:")):
        cases = [
            (b"null", (None, cp, opp, 0, 1, 2, tp, -1, op)),
            (b"null", (handle, None, opp, 0, 1, 2, tp, -1, op)),
            (b"null", (handle, cp, None, 0, 1, 2, tp, -1, op)),
            (b"null", (handle, cp, opp, 0, 1, 2, None, -1, op)),
            (b"null", (handle, cp, opp, 0, 1, 2, tp, -1, None)),
            (b"passes", (handle, cp, opp, 0, 0, 2, tp, -1, op)),
            (b"passes", (handle, cp, opp, 5, -1, 2, tp, -1, op)),
            (b"num_groups", (handle, cp, opp, 0, 1, 0, tp, -1, op)),
            (b"num_groups", (handle, cp, opp, 0, 1, 9, tp, -1, op)),
            (b"num_groups", (handle, cp, opp, 0, 1, -1, tp, -1, op)),
            (b"env_group", (handle, cp, opp, 0, 1, 2, tp, 2, op)),
            (b"env_group", (handle, cp, opp, 0, 1, 2, tp, -2, op)),
            (b"mode", (handle, cp, C.byref(normals), 0, 1, 2, tp, -1, op)),
            (b"tinsel_hip_init", (handle, cp, opp, 0, 1, 2, tp, -1, op)),        # no init
        ]
        for cause, case in cases:
            assert L.tinsel_hip_init(None, 0, 0) == -1 and L.tinsel_hip_last_error().startswith(b"init:")      # another entry's text in between
            assert fn(*case) == -1, case
            msg = L.tinsel_hip_last_error()
            assert msg.startswith(own) and cause in msg, msg
            assert (out == 5.0).all()


def test_default_light_groups():
    veach = tinsel_amd.Scene(lg.pack_bytes("veach"))
    table, env, names = tinsel_amd.default_light_groups(veach)
    assert table.dtype == np.int32 and table.tolist() == [-1, -1, -1, -1, -1, 0, 1, 2, 3] and env == -1 and names == ["prim5", "prim6", "prim7", "prim8"]
    features = tinsel_amd.Scene(lg.pack_bytes("features"))
    table, env, names = tinsel_amd.default_light_groups(features)
    assert table.tolist() == [-1, -1, 0, 1, -1, -1, -1, -1, -1] and env == 2 and names == ["prim2", "prim3", "env"]
    # the probe is an environment too
    assert tinsel_amd.default_light_groups(tinsel_amd.Scene(lg.pack_bytes("features_probe")))[1] == 2
    # nine emitters, eight groups: the last light group takes the overflow
    blob = lg.pack_bytes("veach")
    for i in range(9):
        blob = lg.with_emission(blob, i, (1.0, 0.5, 0.25))
    assert lg.emitters(blob) == list(range(9))
    table, env, names = tinsel_amd.default_light_groups(tinsel_amd.Scene(blob))
    assert table.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 7] and env == -1 and names == ["prim%d" % i for i in range(7)] + ["prim7+"]
    # fewer groups than the scene would fill: lights first, the environment keeps its own
    table, env, names = tinsel_amd.default_light_groups(features, max_groups=2)
    assert table.tolist() == [-1, -1, 0, 0, -1, -1, -1, -1, -1] and env == 1 and names == ["prim2+", "env"]
    for bad in (0, 9):
        with pytest.raises(ValueError):
            tinsel_amd.default_light_groups(veach, max_groups=bad)


def test_relight():
    rng = np.random.default_rng(7)
    planes = rng.random((3, 5, 4, 4)).astype(np.float32)
    one = tinsel_amd.relight(planes, [1.0, 1.0, 1.0])
    assert one.dtype == np.float32 and one.shape == (5, 4, 4)
    assert np.array_equal(one[..., :3], planes[0, ..., :3] + planes[1, ..., :3] + planes[2, ..., :3])      # the plain sum, groups ascending
    assert np.array_equal(one[..., 3], planes[0, ..., 3])                                                     # plane 0's weight: an accumulator
    off = tinsel_amd.relight(planes, [0.0, 2.0, 0.0])
    assert np.array_equal(off[..., :3], planes[0, ..., :3]*np.float32(0) + planes[1, ..., :3]*np.float32(2) + planes[2, ..., :3]*np.float32(0))
    tint = tinsel_amd.relight(planes, [[1.0, 0.5, 0.0], [0.0, 0.0, 0.0], [0.25, 0.25, 0.25]])
    want = planes[0, ..., :3]*np.array([1.0, 0.5, 0.0], np.float32) + planes[1, ..., :3]*np.float32(0) + planes[2, ..., :3]*np.float32(0.25)
    assert np.array_equal(tint[..., :3], want)
    for bad in ([1.0, 1.0], [[1.0, 1.0]]*3, 1.0):
        with pytest.raises(ValueError):
            tinsel_amd.relight(planes, bad)


def test_masked_pack_is_a_byte_edit():
    for name in ("veach", "features", "features_probe"):
        blob = lg.pack_bytes(name)
        assert lg.masked_pack(blob, lg.emitters(blob), True) == blob, name                  # every emitter kept: the input bytes
        dark = lg.masked_pack(blob, (), False)
        assert lg.emitters(dark) == [] and not lg.has_sky(dark) and len(dark) == len(blob)
        differ = np.nonzero(np.frombuffer(dark, np.uint8) != np.frombuffer(blob, np.uint8))[0]
        at = lg.header(blob).off_primitives
        assert all((a < 120 and a >= 96) or (a >= at and (a - at) % 272 - 136 in range(12)) for a in differ.tolist()), name
    blob = lg.pack_bytes("veach")
    one = lg.masked_pack(blob, [6], True)
    assert lg.emitters(one) == [6] and np.array_equal(lg.emission(one, 6), lg.emission(blob, 6))
    assert lg.emitters(blob) == [5, 6, 7, 8] and not lg.has_sky(blob) and lg.has_sky(lg.pack_bytes("features"))


@pytest.mark.parametrize("name", ["veach", "features", "many_spheres"])
def test_the_yardstick_holds_for_the_reference_alone(name):
    """clamp = FLT_MAX: the oracle's masked renders carry the beauty's weight plane, are finite, and add up to the beauty within the bound"""
    blob = lg.pack_bytes(name)
    cam, opt = lg.frame(blob, W, H, clamp=FLT_MAX)
    beauty = lg.oracle_render(blob, cam, opt, 0, PASSES)
    masks = [([i], False) for i in lg.emitters(blob)] + ([((), True)] if lg.has_sky(blob) else [])
    assert len(masks) >= 3
    planes = [lg.oracle_render(lg.masked_pack(blob, keep, sky), cam, opt, 0, PASSES) for keep, sky in masks]
    total = np.zeros(beauty.shape[:2] + (3,), np.float64)
    for p in planes:
        assert np.isfinite(p).all() and np.array_equal(p[..., 3].view(np.uint32), beauty[..., 3].view(np.uint32)), name
        assert (p[..., :3] >= 0).all() and p[..., :3].any()
        total += p[..., :3]
    b = beauty[..., :3].astype(np.float64)
    bound = lg.rounding_c(opt.max_depth, PASSES)*(total + b)
    worst = float((np.abs(total - b)/np.where(bound > 0, bound, 1.0)).max())
    print("%s: %d planes, worst |sum - beauty| = %.3f of the bound" % (name, len(planes), worst))
    assert (np.abs(total - b) <= bound).all(), worst


def test_the_headless_options():
    cfg = headless.parse_args(["headless", "-lightgroups=g.npz", "-lightgroups_spp=5", "-spp=8", "scene.pack"])
    assert (cfg["lightgroups"], cfg["lightgroups_spp"]) == ("g.npz", 5) and cfg["over"] == {"spp": 8}
    cfg = headless.parse_args(["headless", "-lightgroups=g.npz", "scene.pack"])
    assert cfg["lightgroups_spp"] is None                   # min(spp, 16), once the scene's options are known
    assert headless.parse_args(["headless", "scene.pack"])["lightgroups"] is None
    for bad in ("-lightgroups_spp=0", "-lightgroups_spp=-2"):
        with pytest.raises(SystemExit):
            headless.parse_args(["headless", "-lightgroups=g.npz", bad, "scene.pack"])
    with pytest.raises(SystemExit, match="goes with -lightgroups"):
        headless.main(["headless", "-lightgroups_spp=4", "no_such_scene.pack"])
    assert "-lightgroups=FILE.npz" in headless.__doc__ and "-lightgroups_spp" in headless.__doc__

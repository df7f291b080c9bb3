"""CPU tests of the depth-plane boundary (tinsel_hip_render_depth_planes / _device): the declarations in the header and the ctypes mirror,
the three k_shade_depths instances in the launch list and in the library, the refusals that need no GPU, depth_contributions on hand-made
planes, the headless options -- and the yardstick itself, held for the reference alone: the oracle's renders at every depth are finite,
carry one weight plane, never decrease without a clamp, change from depth to depth, and on motionblur change in few pixels (most of its
paths end at the first bounce: the scene that shows a deeper plane an early-ending path failed to fill)."""
import ctypes as C
import functools
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
    assert re.search(r"#define TINSEL_MAX_DEPTH_PLANES\s+16\b", HEADER) and abi.MAX_DEPTH_PLANES == 16
    assert re.search(r"#define TINSEL_MAX_PLANE_DEPTH\s+64\b", HEADER) and abi.MAX_PLANE_DEPTH == 64
    assert re.search(r"#define TINSEL_DEPTH_PLANES_ADD\s+1\b", HEADER) and abi.DEPTH_PLANES_ADD == 1
    assert re.search(r"#define TINSEL_DEPTH_PLANES_ACCUMULATE_SINGLY\s+2\b", HEADER) and abi.DEPTH_PLANES_ACCUMULATE_SINGLY == 2
    for name, tail in (("tinsel_hip_render_depth_planes", r"float\* out_host"), ("tinsel_hip_render_depth_planes_device", r"float\* out_dev, void\* stream")):
        assert hasattr(L, name) and name in tinsel_amd.renderer.EXPORTED_SYMBOLS
        assert re.search(r"\bint %s\(tinsel_hip\* r, const tinsel_camera\* camera, const tinsel_options\* options,\s*uint32_t pass_begin, int passes, "
                         r"int num_planes, const int32_t\* depths, int flags,\s*%s\);" % (name, tail), HEADER), name
    host, dev = L.tinsel_hip_render_depth_planes.argtypes, L.tinsel_hip_render_depth_planes_device.argtypes
    assert list(host) == abi.RENDER_DEPTH_PLANES_ARGTYPES and list(dev) == abi.RENDER_DEPTH_PLANES_DEVICE_ARGTYPES
    assert len(host) == 9 and len(dev) == 10 and list(dev[:9]) == list(host) and dev[9] is C.c_void_p
    assert host[3] is C.c_uint32 and host[4] is host[5] is host[7] is C.c_int and host[0] is host[6] is host[8] is C.c_void_p
    assert callable(tinsel_amd.HipRenderer.depth_planes) and callable(tinsel_amd.depth_contributions)
    # the header states the definition, its consequences and what the call leaves alone
    for text in ("with options->max_depth replaced by depths[k]", "options->max_depth is not read", "applies to EACH PLANE SEPARATELY",
                 "roulette after bounce b changes only what comes later", "the weight channel of every plane is the beauty's",
                 "equal [0, b) in one call, bit for bit", 'timed under the name "k_shade"', "16 bytes x num_planes per path slot",
                 "strictly ascending", "written exactly once"):
        assert text in HEADER, text


def test_the_instances_are_in_the_launch_list_and_in_the_library():
    blob = open(tinsel_amd.renderer.LIB_PATH, "rb").read()
    # (compiled in the tolerance arm's translation unit too, never reached there: the call refuses that arm)
    for ns in (b"_ZN2tn", b"_ZN7tn_fast"):
        for inst in (b"ILb1ELb1EEE", b"ILb1ELb0EEE", b"ILb0ELb0EEE"):
            assert ns + b"14k_shade_depths" + inst in blob, (ns, inst)
    launch = open(os.path.join(ROOT, "tinsel_amd", "csrc", "tn_launch.h")).read()
    assert re.search(r"X\(PK_SHADE_DEPTHS_MIXED,\s+kBlock, 0, SHADE_DEPTHS,\s*k_shade_depths<true, true>\)", launch)
    assert re.search(r"X\(PK_SHADE_DEPTHS_LDS,\s+kBlock, 0, SHADE_DEPTHS,\s*k_shade_depths<true>\)", launch)
    assert re.search(r"X\(PK_SHADE_DEPTHS,\s+kBlock, 0, SHADE_DEPTHS,\s*k_shade_depths<false>\)", launch)
    assert "#define TN_ARGS_SHADE_DEPTHS TN_ARGS_SHADE, a.depths" in launch
    # the planes have one writer per record: no atomics in the shading half of a path
    split = open(os.path.join(ROOT, "tinsel_amd", "csrc", "tn_split.h")).read()
    shade = split[split.index("TN_D bool shade_path"):split.index("__global__ __launch_bounds__(kBlock, TN_WAVES_SHADE) void k_shade(")]
    assert "if constexpr (DEPTHS)" in shade and "atomic" not in shade


def test_refusals_that_need_no_gpu():
    """(the arguments are judged before the renderer is looked at: a handle that is only non-null will do -- zeroed, it was never init-ed)"""
    L = tinsel_amd.load_library()
    out = np.full(16*4*4*4, 5.0, np.float32)
    op = out.ctypes.data_as(C.c_void_p)

    def table(*d):
        a = np.array(d, np.int32)
        return a, a.ctypes.data_as(C.c_void_p)

    two = table(1, 2)                   # (every table stays referenced while its pointer is in use)
    handle = C.create_string_buffer(1 << 20)
    cam, opt, normals = abi.Camera(), abi.Options(), abi.Options()
    opt.mode, opt.width, opt.height = abi.MODE_PATHTRACE, 4, 4
    normals.mode, normals.width, normals.height = abi.MODE_NORMALS, 4, 4
    cp, opp, tp = C.byref(cam), C.byref(opt), two[1]
    bad_lists = [table(0, 2), table(2, 2), table(3, 2), table(1, 65), table(-1, 4)]
    seventeen = table(*range(1, 18))
    host = lambda *a: L.tinsel_hip_render_depth_planes(*a)
    dev = lambda *a: L.tinsel_hip_render_depth_planes_device(*a, None)
    for fn, own in ((host, b"render_depth_planes:"), (dev, b"render_depth_planes_device:")):
        cases = [
            (b"null", (None, cp, opp, 0, 1, 2, tp, 0, op)),
            (b"null", (handle, None, opp, 0, 1, 2, tp, 0, op)),
            (b"null", (handle, cp, None, 0, 1, 2, tp, 0, op)),
            (b"null", (handle, cp, opp, 0, 1, 2, None, 0, op)),
            (b"null", (handle, cp, opp, 0, 1, 2, tp, 0, None)),
            (b"passes", (handle, cp, opp, 0, 0, 2, tp, 0, op)),
            (b"passes", (handle, cp, opp, 5, -1, 2, tp, 0, op)),
            (b"num_planes", (handle, cp, opp, 0, 1, 0, tp, 0, op)),
            (b"num_planes", (handle, cp, opp, 0, 1, 17, seventeen[1], 0, op)),
            (b"num_planes", (handle, cp, opp, 0, 1, -1, tp, 0, op)),
            (b"flag", (handle, cp, opp, 0, 1, 2, tp, 4, op)),
            (b"flag", (handle, cp, opp, 0, 1, 2, tp, -1, op)),
            (b"mode", (handle, cp, C.byref(normals), 0, 1, 2, tp, 0, op)),
            (b"tinsel_hip_init", (handle, cp, opp, 0, 1, 2, tp, 0, op)),        # no init
        ] + [(b"depths[", (handle, cp, opp, 0, 1, 2, t[1], 0, op)) for t in bad_lists]
        for cause, case in cases:
            assert L.tinsel_hip_init(None, 0, 0) == -1 and L.tinsel_hip_last_error().startswith(b"init:")      # another entry's text in between
            assert fn(*case) == -1, case
            msg = L.tinsel_hip_last_error()
            assert msg.startswith(own) and cause in msg, msg
            assert (out == 5.0).all()


def test_depth_contributions():
    # 3 planes of 1 x 3 pixels: weights 2, 0.5 and 0 (a pixel no sample reached)
    planes = np.zeros((3, 1, 3, 4), np.float32)
    planes[:, 0, :, 3] = [2.0, 0.5, 0.0]
    planes[0, 0, 0, :3] = [2.0, 4.0, 0.0]
    planes[1, 0, 0, :3] = [3.0, 4.0, 1.0]
    planes[2, 0, 0, :3] = [3.0, 8.0, 1.0]
    planes[0, 0, 1, :3] = [1.0, 0.0, 0.25]
    planes[1, 0, 1, :3] = [0.5, 0.0, 0.25]             # a finite clamp: a deeper plane below a shallower one
    planes[2, 0, 1, :3] = [0.5, 1.0, 0.25]
    planes[:, 0, 2, :3] = 7.0                           # colour without weight: 0, not inf or nan
    c = tinsel_amd.depth_contributions(planes)
    assert c.dtype == np.float32 and c.shape == (3, 1, 3, 3) and np.isfinite(c).all()
    assert c[:, 0, 0].tolist() == [[1.0, 2.0, 0.0], [0.5, 0.0, 0.5], [0.0, 2.0, 0.0]]
    assert c[:, 0, 1].tolist() == [[2.0, 0.0, 0.5], [-1.0, 0.0, 0.0], [0.0, 2.0, 0.0]]
    assert not c[:, 0, 2].any()
    # the shares add up to the deepest plane's image; one plane is its image
    assert np.array_equal(c.sum(axis=0)[0, :2], planes[2, 0, :2, :3]/planes[2, 0, :2, 3:4])
    one = tinsel_amd.depth_contributions(planes[:1])
    assert one.shape == (1, 1, 3, 3) and np.array_equal(one[0], c[0])
    for bad in (planes[0], planes[..., :3], np.zeros((0, 1, 3, 4), np.float32)):
        with pytest.raises(ValueError):
            tinsel_amd.depth_contributions(bad)
    assert "negative" in tinsel_amd.depth_contributions.__doc__ and "clamp" in tinsel_amd.depth_contributions.__doc__


def test_the_headless_options():
    cfg = headless.parse_args(["headless", "-depthplanes=d.npz", "-depthplanes_spp=5", "-depthplanes_at=1,2,8", "-spp=8", "scene.pack"])
    assert (cfg["depthplanes"], cfg["depthplanes_spp"], cfg["depthplanes_at"]) == ("d.npz", 5, (1, 2, 8)) and cfg["over"] == {"spp": 8}
    cfg = headless.parse_args(["headless", "-depthplanes=d.npz", "scene.pack"])
    assert cfg["depthplanes_spp"] is None and cfg["depthplanes_at"] is None        # min(spp, 16) and 1 .. max depth, once the scene's options are known
    assert headless.parse_args(["headless", "scene.pack"])["depthplanes"] is None
    many = ",".join(str(d) for d in range(1, 18))
    for bad in ("-depthplanes_spp=0", "-depthplanes_spp=-2", "-depthplanes_at=0,1", "-depthplanes_at=2,2", "-depthplanes_at=3,1", "-depthplanes_at=1,65",
                "-depthplanes_at=", "-depthplanes_at=1,x", "-depthplanes_at=" + many):
        with pytest.raises(SystemExit):
            headless.parse_args(["headless", "-depthplanes=d.npz", bad, "scene.pack"])
    for alone in ("-depthplanes_spp=4", "-depthplanes_at=1,2"):
        with pytest.raises(SystemExit, match="go with -depthplanes"):
            headless.main(["headless", alone, "no_such_scene.pack"])
    # the exclusions of -lightgroups
    for other in ("-resume=s.npz", "-complexity=rays", "-firsthit=f.npz", "-irradiance=i.npz"):
        with pytest.raises(SystemExit, match="-depthplanes writes the depth planes of a normal render"):
            headless.main(["headless", "-depthplanes=d.npz", other, "no_such_scene.pack"])
    with pytest.raises(SystemExit, match="-depthplanes writes the depth planes of a normal render"):
        headless.main(["headless", "-depthplanes=d.npz", "no_such_scene_%d.pack"])
    for text in ("-depthplanes=FILE.npz", "-depthplanes_spp", "-depthplanes_at", "`planes`", "`depths`", "`passes`"):
        assert text in headless.__doc__, text


def test_depth_planes_refuses_more_depths_than_planes_without_a_gpu():
    """depths=None means 1 .. options.max_depth: more than 16 is refused before the library is asked"""
    opt = abi.Options()
    opt.mode, opt.width, opt.height, opt.max_depth = abi.MODE_PATHTRACE, 4, 4, 17
    with pytest.raises(ValueError, match="name the depths"):
        tinsel_amd.HipRenderer.depth_planes(None, abi.Camera(), opt, 0, 1)


@functools.lru_cache(maxsize=None)
def _oracle_at(name, depth):
    blob = lg.pack_bytes(name)
    cam, opt = lg.frame(blob, W, H, clamp=FLT_MAX)
    opt.max_depth = depth
    return lg.oracle_render(blob, cam, opt, 0, PASSES)


@pytest.mark.parametrize("name", ["cornell", "veach", "glass", "features_probe", "motionblur"])
def test_the_yardstick_holds_for_the_reference_alone(name):
    """clamp = FLT_MAX: the oracle's renders at the depths 1 .. max(4, the scene's own) are finite, carry one weight plane, never decrease
    from depth to depth (every term is non-negative and fp32 addition is monotone) and change in at least one pixel at every step"""
    own = int(lg.frame(lg.pack_bytes(name), W, H)[1].max_depth)
    D = max(4, own)
    renders = [_oracle_at(name, d) for d in range(1, D + 1)]
    changed = []
    for d, (a, b) in enumerate(zip(renders, renders[1:]), 1):
        assert np.isfinite(a).all() and np.isfinite(b).all(), (name, d)
        assert np.array_equal(a[..., 3].view(np.uint32), b[..., 3].view(np.uint32)), (name, d)
        assert (b[..., :3] >= a[..., :3]).all(), (name, d)
        changed.append(int((a != b).any(axis=-1).sum()))
    print("%s: depths 1 .. %d, pixels changed per step: %s" % (name, D, changed))
    assert renders[0][..., :3].any() and all(n >= 1 for n in changed), changed
    if name == "motionblur":
        # most paths end at the first bounce: the fill of deeper planes by a path that ended is exercised
        assert changed[0] < W*H//4, changed

"""CPU tests of the feature-buffer boundary (tinsel_hip_render_features / _device): the declarations and the three bits in the header, the
ctypes mirror, the kernel in the launch list, the name table and the library under both arithmetic contracts, the refusals that need no
GPU, feature_images on hand-made planes, and the headless options."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tinsel_amd
from tinsel_amd import abi, headless

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "tinsel_hip.h")).read()


def test_the_entries_and_the_bits_are_declared_exported_and_bound():
    L = tinsel_amd.load_library()
    for name, bit in (("ALBEDO", 1), ("NORMAL", 2), ("DEPTH", 4)):
        assert re.search(r"#define TINSEL_FEATURE_%s\s+%du\b" % (name, bit), HEADER)
        assert getattr(abi, "FEATURE_" + name) == bit
    assert abi.FEATURE_NAMES == ("albedo", "normal", "depth")
    for name, out in (("tinsel_hip_render_features", "out_host"), ("tinsel_hip_render_features_device", "out_dev, void\\* stream")):
        assert hasattr(L, name) and name in tinsel_amd.renderer.EXPORTED_SYMBOLS
        assert re.search(r"\bint %s\(tinsel_hip\* r, const tinsel_camera\* camera, const tinsel_options\* options,\s*uint32_t pass_begin, int passes, "
                         r"unsigned features, float\* %s\);" % (name, out), HEADER)
    host, dev = L.tinsel_hip_render_features.argtypes, L.tinsel_hip_render_features_device.argtypes
    assert len(host) == 7 and len(dev) == 8 and dev[:7] == host and dev[7] is C.c_void_p
    assert host[3] is C.c_uint32 and host[4] is C.c_int and host[5] is C.c_uint and host[0] is C.c_void_p and host[6] is C.c_void_p
    assert callable(tinsel_amd.HipRenderer.features) and callable(tinsel_amd.feature_images)
    # the header states the buffer sizes and what the planes mean
    for text in ("16 bytes x popcount(features) per path slot of a batch", "max(1, floor(batch_paths / slots per pass))", "z/w is the coverage"):
        assert text in HEADER, text
    assert tinsel_amd.feature_mask(("depth", "albedo")) == (5, ["albedo", "depth"]) and tinsel_amd.feature_mask("normal") == (2, ["normal"])
    assert tinsel_amd.feature_mask(abi.FEATURE_NAMES)[0] == 7 and tinsel_amd.feature_mask(())[0] == 0
    with pytest.raises(ValueError):
        tinsel_amd.feature_mask(("albedo", "colour"))


def test_the_kernel_is_in_the_library_under_both_arithmetic_contracts():
    blob = open(tinsel_amd.renderer.LIB_PATH, "rb").read()
    for ns in (b"_ZN2tn", b"_ZN7tn_fast"):
        assert ns + b"10k_featuresILb1EEE" in blob and ns + b"10k_featuresILb0EEE" in blob
    launch = open(os.path.join(ROOT, "tinsel_amd", "csrc", "tn_launch.h")).read()
    assert re.search(r"X\(PK_FEATURES_LDS,\s+kBlock, 0, FEATURES,\s*k_features<true>\)", launch)
    assert re.search(r"X\(PK_FEATURES,\s+kBlock, 0, FEATURES,\s*k_features<false>\)", launch)
    layout = open(os.path.join(ROOT, "tinsel_amd", "csrc", "tn_host_layout.h")).read()
    names = re.search(r"kKernelNames\[\] = \{([^}]*)\}", layout).group(1).replace('"', "").split(",")
    ids = re.search(r"enum \{ KN_GENERATE = 0,([^}]*)KN_COUNT \}", layout).group(1).split(",")
    names, ids = [s.strip() for s in names], ["KN_GENERATE"] + [s.strip() for s in ids if s.strip()]
    assert len(names) == len(ids) and names.index("k_features") == ids.index("KN_FEATURES") == len(names) - 1
    # appended: the entries in front of it are where they were
    assert names[-2] == "k_gather_sh_reduce" and ids[-2] == "KN_GATHER_SH_REDUCE"


def test_refusals_that_need_no_gpu():
    """(the arguments are judged before the renderer is looked at: a handle that is only non-null will do -- zeroed, it was never init-ed)"""
    L = tinsel_amd.load_library()
    out = np.full(3*4*4*4, 5.0, np.float32)
    op = out.ctypes.data_as(C.c_void_p)
    handle = C.create_string_buffer(1 << 20)
    cam, opt, normals = abi.Camera(), abi.Options(), abi.Options()
    opt.mode, opt.width, opt.height = abi.MODE_PATHTRACE, 4, 4
    normals.mode, normals.width, normals.height = abi.MODE_NORMALS, 4, 4
    cp, opp = C.byref(cam), C.byref(opt)
    host = lambda *a: L.tinsel_hip_render_features(*a)
    dev = lambda *a: L.tinsel_hip_render_features_device(*a, None)
    for fn, own in ((host, b"render_features:"), (dev, b"render_features_device:")):
        cases = [
            (b"null", (None, cp, opp, 0, 1, 7, op)),
            (b"null", (handle, None, opp, 0, 1, 7, op)),
            (b"null", (handle, cp, None, 0, 1, 7, op)),
            (b"null", (handle, cp, opp, 0, 1, 7, None)),
            (b"passes", (handle, cp, opp, 0, 0, 7, op)),
            (b"passes", (handle, cp, opp, 5, -1, 7, op)),
            (b"features", (handle, cp, opp, 0, 1, 0, op)),
            (b"features", (handle, cp, opp, 0, 1, 8, op)),
            (b"features", (handle, cp, opp, 0, 1, 0xffffffff, op)),
            (b"mode", (handle, cp, C.byref(normals), 0, 1, 7, op)),
            (b"tinsel_hip_init", (handle, cp, opp, 0, 1, 7, op)),        # no init
        ]
        for cause, case in cases:
            assert L.tinsel_hip_init(None, 0, 0) == -1 and L.tinsel_hip_last_error().startswith(b"init:")      # another entry's text in between
            assert fn(*case) == -1, case
            msg = L.tinsel_hip_last_error()
            assert msg.startswith(own) and cause in msg, msg
            assert (out == 5.0).all()


def test_feature_images_on_hand_made_planes():
    H, W = 2, 3
    albedo, normal, depth = (np.zeros((H, W, 4), np.float32) for _ in range(3))
    # pixel (0, 0): weight 2, two hits at depths 3 and 5 with equal weights
    albedo[0, 0] = [0.5, 1.0, 1.5, 2.0]
    normal[0, 0] = [0.0, 0.0, 4.0, 2.0]
    depth[0, 0] = [3.0 + 5.0, 9.0 + 25.0, 2.0, 2.0]
    # pixel (0, 1): weight 4, half of it hit; the normals cancel
    albedo[0, 1] = [1.0, 0.0, 0.0, 4.0]
    normal[0, 1] = [0.0, 0.0, 0.0, 4.0]
    depth[0, 1] = [7.0*2.0, 49.0*2.0, 2.0, 4.0]
    # pixel (0, 2): weight, but no sample hit anything (z == 0)
    albedo[0, 2] = normal[0, 2] = depth[0, 2] = [0.0, 0.0, 0.0, 1.5]
    # pixel (1, 0): no weight at all (w == 0); pixel (1, 1): a tilted normal
    normal[1, 1] = [3.0, 0.0, 4.0, 10.0]
    albedo[1, 1] = [0.25, 0.25, 0.25, 10.0]
    depth[1, 1] = [10.0, 10.0, 10.0, 10.0]
    im = tinsel_amd.feature_images({"albedo": albedo, "normal": normal, "depth": depth})
    assert sorted(im) == ["albedo", "coverage", "depth", "depth_variance", "normal"]
    assert all(v.dtype == np.float64 for v in im.values())
    assert im["albedo"].shape == im["normal"].shape == (H, W, 3) and im["depth"].shape == im["depth_variance"].shape == im["coverage"].shape == (H, W)
    assert np.array_equal(im["albedo"][0, 0], [0.25, 0.5, 0.75]) and np.array_equal(im["albedo"][0, 1], [0.25, 0.0, 0.0])
    assert np.array_equal(im["normal"][0, 0], [0.0, 0.0, 1.0]) and np.array_equal(im["normal"][0, 1], [0.0, 0.0, 0.0])
    assert np.allclose(im["normal"][1, 1], [0.6, 0.0, 0.8], rtol=1e-15, atol=0)
    assert im["depth"][0, 0] == 4.0 and im["depth_variance"][0, 0] == 1.0 and im["coverage"][0, 0] == 1.0
    assert im["depth"][0, 1] == 7.0 and im["depth_variance"][0, 1] == 0.0 and im["coverage"][0, 1] == 0.5
    assert im["depth"][1, 1] == 1.0 and im["depth_variance"][1, 1] == 0.0 and im["coverage"][1, 1] == 1.0
    # z == 0: no depth, no variance, coverage 0, albedo and normal 0
    for k in ("depth", "depth_variance", "coverage"):
        assert im[k][0, 2] == 0.0 and im[k][1, 0] == 0.0 and im[k][1, 2] == 0.0
    for k in ("albedo", "normal"):
        assert not im[k][0, 2].any() and not im[k][1, 0].any()
    assert all(np.isfinite(v).all() for v in im.values())
    # only the planes that are there
    assert sorted(tinsel_amd.feature_images({"normal": normal})) == ["normal"]
    assert sorted(tinsel_amd.feature_images({"depth": depth})) == ["coverage", "depth", "depth_variance"]


def test_the_headless_options():
    cfg = headless.parse_args(["headless", "-features=f.npz", "-features_spp=5", "-spp=8", "scene.pack"])
    assert (cfg["features"], cfg["features_spp"]) == ("f.npz", 5) and cfg["over"] == {"spp": 8}
    cfg = headless.parse_args(["headless", "-features=f.npz", "scene.pack"])
    assert cfg["features_spp"] is None                      # min(spp, 16), once the scene's options are known
    assert headless.parse_args(["headless", "scene.pack"])["features"] is None
    for bad in ("-features_spp=0", "-features_spp=-2"):
        with pytest.raises(SystemExit):
            headless.parse_args(["headless", "-features=f.npz", bad, "scene.pack"])
    # it goes with a normal render of passes [0, N): refused beside what renders none or starts elsewhere, before the scene is opened
    for other in ("-resume=s.npz", "-complexity=rays", "-irradiance=i.npz", "-firsthit=b.npz"):
        with pytest.raises(SystemExit, match="-features writes"):
            headless.main(["headless", "-features=f.npz", other, "no_such_scene.pack"])
    with pytest.raises(SystemExit, match="-features writes"):
        headless.main(["headless", "-features=f.npz", "-probes=p.npz", "-probes_at=at.npy", "no_such_scene.pack"])
    with pytest.raises(SystemExit, match="-features writes"):
        headless.main(["headless", "-features=f.npz", "no_such_%d.pack"])
    with pytest.raises(SystemExit, match="goes with -features"):
        headless.main(["headless", "-features_spp=4", "no_such_scene.pack"])
    assert "-features=FILE.npz" in headless.__doc__ and "-features_spp" in headless.__doc__

"""Depth planes (tinsel_hip_render_depth_planes / _device, kernel k_shade_depths): the beauty at several path depths in one trace.

The yardstick is not under test: plane k is, bit for bit in all four channels, the oracle's render of the same pack with max_depth replaced
by depths[k] (tests/light_groups_reference.py's oracle_render; the oracle is the one the parity tests use).  Every case renders 48 x 32
pixels, 4 passes from pass 0, with the pack's own options unless it says otherwise; oracle renders are computed once, shared and left
unchanged, and every one a plane is compared with is asserted finite and not all zero.

Figures (MI355X): the cases are bit-for-bit and have none."""
import ctypes as C
import functools

import numpy as np
import pytest

import tinsel_amd
from tinsel_amd import abi
from tests import light_groups_reference as lg

pytestmark = pytest.mark.gpu

W, H, PASSES = 48, 32, 4
PIPELINES = {"auto": abi.PIPELINE_AUTO, "wavefront": abi.PIPELINE_WAVEFRONT, "mega": abi.PIPELINE_MEGAKERNEL, "split": abi.PIPELINE_WAVEFRONT_SPLIT,
             "paired": abi.PIPELINE_WAVEFRONT_PAIRED}


@functools.lru_cache(maxsize=None)
def _blob(name):
    return lg.pack_bytes(name)


@functools.lru_cache(maxsize=None)
def _oracle(name, depth, width=W, height=H, pass_begin=0, passes=PASSES):
    """the oracle's render of the pack with max_depth = depth: the yardstick of one plane"""
    cam, opt = lg.frame(_blob(name), width, height)
    opt.max_depth = depth
    out = lg.oracle_render(_blob(name), cam, opt, pass_begin, passes)
    assert np.isfinite(out).all() and out[..., :3].any(), (name, depth)
    return out


def _open(name, width=W, height=H):
    scene = tinsel_amd.Scene(_blob(name))
    r = tinsel_amd.create_gpu_renderer(scene)
    r.init(width, height)
    cam, opt = lg.frame(_blob(name), width, height)
    return scene, r, cam, opt


def _own_depth(name):
    return int(lg.frame(_blob(name), W, H)[1].max_depth)


def _same(got, want, what):
    assert got.dtype == np.float32 and got.shape == want.shape, what
    bad = (got != want).any(axis=-1)
    first = np.unravel_index(np.argmax(bad), bad.shape)
    assert np.array_equal(got, want), "%s: %d of %d pixels differ (first: %s, %s against %s)" % (what, int(bad.sum()), bad.size, first, got[first], want[first])


def _same_planes(planes, name, depths, what, **frame):
    assert planes.shape[0] == len(depths), what
    for k, d in enumerate(depths):
        _same(planes[k], _oracle(name, d, **frame), "%s, plane %d = depth %d" % (what, k, d))


# ---------------------------------------------------------------------------
# 1: exact, per plane, against the oracle's render at that depth

# scene, D (the planes are the depths 1 .. D), frame
CASES = {
    "cornell": ("cornell", 4, {}),                                  # closed, the flat scan
    "veach": ("veach", 4, {}),                                      # a finite clamp, lights with several samples
    "glass": ("glass", 8, {}),                                      # media
    "features_probe": ("features_probe", 6, {}),                    # probe light samples and the miss branch's MIS weight
    "motionblur": ("motionblur", 4, {}),                            # a moving mesh light, meshes in HBM, early ends
    "many_spheres": ("many_spheres", 4, {}),                        # the scene-level walk
    "veach_50x34": ("veach", 4, {"width": 50, "height": 34}),       # ragged tiles
    "veach_pass3": ("veach", 4, {"pass_begin": 3}),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_plane_is_the_oracles_render_at_its_depth(case):
    name, D, how = CASES[case]
    width, height, pass_begin = how.get("width", W), how.get("height", H), how.get("pass_begin", 0)
    depths = list(range(1, D + 1))
    scene, r, cam, opt = _open(name, width, height)
    try:
        opt.max_depth = 1                                           # not read: the trace runs to depths[last]
        planes = r.depth_planes(cam, opt, pass_begin, PASSES, depths)
    finally:
        r.close()
    assert planes.shape == (D, height, width, 4)
    _same_planes(planes, name, depths, case, width=width, height=height, pass_begin=pass_begin)


def test_depths_none_is_one_to_max_depth():
    scene, r, cam, opt = _open("veach")
    try:
        opt.max_depth = 3
        planes = r.depth_planes(cam, opt, 0, PASSES)
    finally:
        r.close()
    _same_planes(planes, "veach", [1, 2, 3], "veach, depths=None at max_depth 3")


# ---------------------------------------------------------------------------
# 2: sparse and single lists, sixteen planes

@pytest.mark.parametrize("depths", [(1, 8), (2, 3, 8), (8,), (1,)], ids=lambda d: "-".join(str(x) for x in d))
def test_sparse_and_single_depth_lists(depths):
    scene, r, cam, opt = _open("glass")
    try:
        planes = r.depth_planes(cam, opt, 0, PASSES, depths)
        beauty = None
        if depths == (8,):
            assert opt.max_depth == 8
            beauty = r.render(cam, opt, passes=PASSES)
    finally:
        r.close()
    _same_planes(planes, "glass", depths, "glass %s" % (depths,))
    if beauty is not None:
        _same(planes[0], beauty, "glass [8] against tinsel_hip_render")


def test_sixteen_planes():
    depths = list(range(1, 17))
    scene, r, cam, opt = _open("glass")
    try:
        planes = r.depth_planes(cam, opt, 0, PASSES, depths)
    finally:
        r.close()
    _same_planes(planes, "glass", depths, "glass 1 .. 16")


# ---------------------------------------------------------------------------
# 3: roulette, add

def test_roulette_applies_as_in_a_render():
    """after set_russian_roulette(2) each plane is this renderer's own render at that depth (render exists before this call and is not
    under test; the oracle has no roulette)"""
    depths = list(range(1, 9))
    scene, r, cam, opt = _open("glass")
    try:
        r.set_russian_roulette(2)
        planes = r.depth_planes(cam, opt, 0, PASSES, depths)
        renders = []
        for d in depths:
            at = opt.copy()
            at.max_depth = d
            r.write_accum(np.zeros((H, W, 4), np.float32), 0)           # a zeroed accumulator at pass index 0
            renders.append(r.render(cam, at, passes=PASSES))
    finally:
        r.close()
    for k, d in enumerate(depths):
        assert np.isfinite(renders[k]).all() and renders[k][..., :3].any()
        _same(planes[k], renders[k], "glass under roulette from bounce 2, depth %d" % d)
    # (roulette shows from depth 3 on: the planes are not the oracle's there)
    _same(planes[1], _oracle("glass", 2), "glass under roulette, depth 2")
    assert not np.array_equal(planes[7], _oracle("glass", 8))


@functools.lru_cache(maxsize=None)
def _veach_planes():
    scene, r, cam, opt = _open("veach")
    try:
        out = r.depth_planes(cam, opt, 0, PASSES, [1, 2, 3, 4])
    finally:
        r.close()
    out.setflags(write=False)
    _same_planes(out, "veach", [1, 2, 3, 4], "veach 1 .. 4")
    return out


@pytest.mark.parametrize("singly", [False, True], ids=["one_launch", "singly"])
def test_two_calls_with_add_equal_one(singly):
    scene, r, cam, opt = _open("veach")
    try:
        out = r.depth_planes(cam, opt, 0, 2, [1, 2, 3, 4], singly=singly)
        got = r.depth_planes(cam, opt, 2, 2, [1, 2, 3, 4], out=out, add=True, singly=singly)
    finally:
        r.close()
    assert got is out
    _same(out, _veach_planes(), "veach: passes [0, 2) then [2, 4) with add")


# ---------------------------------------------------------------------------
# 4: independence

def test_the_batch_cut_does_not_show():
    scene, r, cam, opt = _open("veach")
    try:
        r.enable_kernel_timing(True)
        r.set_batch_paths(W*H)                      # one pass per batch at the most: four batches
        planes = r.depth_planes(cam, opt, 0, PASSES, [1, 2, 3, 4])
        times = r.kernel_times()
        singly = r.depth_planes(cam, opt, 0, PASSES, [1, 2, 3, 4], singly=True)
        times_singly = r.kernel_times()
    finally:
        r.close()
    _same(planes, _veach_planes(), "veach, one pass per batch")
    _same(singly, _veach_planes(), "veach, one pass per batch, one accumulate launch per plane")
    # four batches: k_generate once each, ONE k_accumulate per batch (per plane and batch singly), k_shade_depths under k_shade's name once
    # per bounce and batch
    assert times["k_generate"][0] == PASSES and times["k_accumulate"][0] == PASSES and times["k_shade"][0] == PASSES*4
    assert times_singly["k_accumulate"][0] == PASSES*4


@pytest.mark.parametrize("pipeline", sorted(PIPELINES))
def test_the_pipeline_setting_does_not_show(pipeline):
    scene, r, cam, opt = _open("veach")
    try:
        r.set_pipeline(PIPELINES[pipeline])
        planes = r.depth_planes(cam, opt, 0, PASSES, [1, 2, 3, 4])
    finally:
        r.close()
    _same(planes, _veach_planes(), "veach under set_pipeline(%s)" % pipeline)


def test_the_device_entry_on_a_callers_stream():
    import torch
    scene, r, cam, opt = _open("veach")
    try:
        out = torch.full((4, H, W, 4), 7.0, dtype=torch.float32, device="cuda:0")
        s = torch.cuda.Stream(device=0)
        s.wait_stream(torch.cuda.current_stream(0))
        with torch.cuda.stream(s):
            got = r.depth_planes(cam, opt, 0, PASSES, [1, 2, 3, 4], out=out)
        s.synchronize()
        assert got is out
        planes = out.cpu().numpy()
        # a render on the default stream afterwards finds the path buffers in order (the fence)
        beauty = r.render(cam, opt, passes=PASSES)
    finally:
        r.close()
    _same(planes, _veach_planes(), "veach, device entry")
    _same(beauty, _oracle("veach", _own_depth("veach")), "the render behind the device entry")


@pytest.mark.parametrize("name", ["veach", "many_spheres"])
def test_a_call_between_two_renders_leaves_no_trace(name):
    def run(with_call):
        scene, r, cam, opt = _open(name)
        try:
            r.render(cam, opt, passes=2)
            before, index = r.stats(), r.get_pass_index()
            planes = r.depth_planes(cam, opt, 0, PASSES, [1, 3, 4]) if with_call else None
            assert r.get_pass_index() == index == 2 and r.stats() == before
            split = r.render(cam, opt, passes=2)
            table, env, _ = tinsel_amd.default_light_groups(scene)
            groups = r.light_groups(cam, opt, 0, PASSES, table, env)
            views = r.views([cam, cam], opt, 0, 2)
        finally:
            r.close()
        return planes, split, groups, views

    planes, split, groups, views = run(True)
    _, split0, groups0, views0 = run(False)
    _same(split, _oracle(name, _own_depth(name)), "%s: 2 passes, a depth-planes call, 2 passes" % name)
    _same(split, split0, "%s: the render behind the call" % name)
    _same(groups, groups0, "%s: a light-groups call behind the call" % name)
    _same(views, views0, "%s: a views call behind the call" % name)
    assert groups[..., :3].any() and views[..., :3].any()
    _same_planes(planes, name, [1, 3, 4], "%s: the call between the renders" % name)


# ---------------------------------------------------------------------------
# 5: refusals

def test_refusals_leave_out_untouched():
    scene, r, cam, opt = _open("veach")
    L = tinsel_amd.load_library()
    try:
        out = np.full((2, H, W, 4), 5.0, np.float32)
        good = np.array([2, 4], np.int32)

        def refused(cause, table=good, flags=0, o=opt, passes=PASSES, planes=2, target=out):
            tp = table.ctypes.data_as(C.c_void_p) if table is not None else None
            op = target.ctypes.data_as(C.c_void_p) if target is not None else None
            rc = L.tinsel_hip_render_depth_planes(r._h, C.byref(cam), C.byref(o), 0, passes, planes, tp, flags, op)
            msg = L.tinsel_hip_last_error()
            assert rc == -1 and msg.startswith(b"render_depth_planes:") and cause in msg, (cause, rc, msg)
            assert (out == 5.0).all(), cause

        refused(b"null", table=None)
        refused(b"null", target=None)
        rc = L.tinsel_hip_render_depth_planes(r._h, None, C.byref(opt), 0, PASSES, 2, good.ctypes.data_as(C.c_void_p), 0, out.ctypes.data_as(C.c_void_p))
        assert rc == -1 and b"null" in L.tinsel_hip_last_error() and (out == 5.0).all()
        rc = L.tinsel_hip_render_depth_planes(r._h, C.byref(cam), None, 0, PASSES, 2, good.ctypes.data_as(C.c_void_p), 0, out.ctypes.data_as(C.c_void_p))
        assert rc == -1 and b"null" in L.tinsel_hip_last_error() and (out == 5.0).all()
        refused(b"passes", passes=0)
        refused(b"num_planes", planes=0)
        refused(b"num_planes", planes=17, table=np.arange(1, 18, dtype=np.int32))
        for bad in ([0, 4], [4, 4], [4, 2], [2, 65]):
            refused(b"depths[", table=np.array(bad, np.int32))
        refused(b"flag", flags=4)
        refused(b"flag", flags=1 | 8)
        other = opt.copy()
        other.width = W + 1
        refused(b"tinsel_hip_init", o=other)
        normals = opt.copy()
        normals.mode = abi.MODE_NORMALS
        refused(b"mode", o=normals)
        r.set_arithmetic(abi.ARITH_FAST)
        refused(b"TINSEL_ARITH_FAST")
        r.set_arithmetic(abi.ARITH_EXACT)
        r.set_shard(0, 2, 16)
        refused(b"sharded")
        r.set_shard(0, 1, 16)
        # the device entry: a misaligned array
        import torch
        dev = torch.full((2*H*W*4 + 4,), 5.0, dtype=torch.float32, device="cuda:0")
        rc = L.tinsel_hip_render_depth_planes_device(r._h, C.byref(cam), C.byref(opt), 0, PASSES, 2, good.ctypes.data_as(C.c_void_p), 0,
                                                     dev.data_ptr() + 4, None)
        assert rc == -1 and b"16-byte aligned" in L.tinsel_hip_last_error()
        torch.cuda.synchronize()
        assert bool((dev == 5.0).all())
        # ... and after all of that the call still works
        planes = r.depth_planes(cam, opt, 0, PASSES, good)
        _same_planes(planes, "veach", [2, 4], "veach [2, 4] after the refusals")
        # a moved primitive without a rebuild
        prims = C.cast(scene.desc.primitives, C.POINTER(abi.Primitive))
        r.set_primitive_transform(0, abi.Transform.from_buffer_copy(bytes(prims[0].start_transform)))
        refused(b"tinsel_hip_rebuild_scene")
    finally:
        r.close()

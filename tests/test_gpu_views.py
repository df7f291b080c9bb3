"""View batches (tinsel_hip_render_views / _device, kernels k_generate_views and k_views_accumulate): the frames of many cameras in one call.

The yardstick is not under test: plane v is, bit for bit in all four channels, the oracle's render_seeded of cameras[v] alone
(tests/views_reference.py; the oracle is the one the parity tests use) -- and, on a second renderer, what init / set_pass_index / render /
read_accum give for that camera.  Every case renders 40 x 24 pixels (three by two accumulate tiles, both edges ragged), 3 passes, 5 views
unless it says otherwise; oracle renders are computed once, shared and left unchanged.  Everything is np.array_equal on the raw floats: no
case has a figure to report."""
import ctypes as C

import numpy as np
import pytest

import tinsel_amd
from tinsel_amd import abi
from tests import views_reference as vr

pytestmark = pytest.mark.gpu

W, H, PASSES = vr.W, vr.H, 3
PACKS = ["cornell", "veach", "glass", "motionblur", "features_probe", "many_spheres", "ajax_standin_96"]
SHUTTERS = [(0.0, 0.15), (0.0, 1.0), (0.5, 0.5), (0.25, 0.75), (0.9, 1.0)]
PIPELINES = {"auto": abi.PIPELINE_AUTO, "wavefront": abi.PIPELINE_WAVEFRONT, "mega": abi.PIPELINE_MEGAKERNEL, "split": abi.PIPELINE_WAVEFRONT_SPLIT,
             "paired": abi.PIPELINE_WAVEFRONT_PAIRED}


def _cameras(name):
    return vr.five_cameras(name, SHUTTERS if name == "motionblur" else None)


def _open(name):
    scene = tinsel_amd.Scene(vr.pack_bytes(name))
    r = tinsel_amd.create_gpu_renderer(scene)
    r.init(W, H)
    _, opt = vr.frame(name)
    return scene, r, opt


def _same(got, want, what, bits=False):
    """np.array_equal on the floats; bits: on their bit patterns (a NaN equals itself, -0 is not +0)"""
    assert got.dtype == np.float32 and got.shape == want.shape, what
    if bits:
        got, want = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    bad = (got != want).any(axis=-1)
    first = np.unravel_index(np.argmax(bad), bad.shape)
    assert np.array_equal(got, want), "%s: %d of %d pixels differ (first: %s, %s against %s)" % (what, int(bad.sum()), bad.size, first, got[first], want[first])


def _render(r, cam, opt, pass_begin, passes, start=None):
    """what tinsel_hip_render gives for one camera from a zeroed accumulator (or `start`) at pass index pass_begin"""
    r.write_accum(np.zeros((H, W, 4), np.float32) if start is None else start, pass_begin)
    r.render(cam, opt, passes=passes, readback=False)
    return r.read_accum()


def _filter(opt, kind, width, falloff=1.0, offset=None):
    out = abi.Options.from_buffer_copy(bytes(opt))
    out.filter.type, out.filter.width, out.filter.falloff = kind, width, falloff
    if offset is not None:
        out.filter.offset = offset
    return out


def _support(opt):
    arg = C.c_float(0.0)
    return bool(tinsel_amd.load_library().tinsel_hip_accumulate_support(opt.filter.type, opt.filter.width, opt.filter.falloff, opt.filter.offset, C.byref(arg)))


# name -> how the pack's options are changed (veach: a finite clamp of 4 that bites)
FILTERS = {
    "own": lambda o: o,                                             # Gaussian 0.75: the compile-time window 3
    "box": lambda o: _filter(o, 0, 0.75),
    "gauss_1": lambda o: _filter(o, 1, 1.0, 1.0, 0.01),             # the compile-time window 4
    "gauss_2": lambda o: _filter(o, 1, 2.0, 0.5, 0.01),             # the run-time window
    "gauss_2_5": lambda o: _filter(o, 1, 2.5, 0.5, 0.01),           # no tiled form: one k_accumulate per view
    "support": lambda o: _filter(o, 1, 0.75, 2.0, 0.3),             # the support rule holds: a render runs its support form, the call the full window
}


# ---------------------------------------------------------------------------
# 1: against the oracle, per view

@pytest.mark.parametrize("name", PACKS)
def test_every_plane_is_the_oracles_render_of_its_camera(name):
    cams = _cameras(name)
    scene, r, opt = _open(name)
    try:
        r.enable_kernel_timing(True)
        planes = r.views(cams, opt, 0, PASSES)
        times = r.kernel_times()
        # one generation and one accumulate launch for the five views; never the fused kernel, which makes the camera's paths itself
        assert times["k_generate"][0] == 1 and times["k_accumulate"][0] == 1 and "k_bounce" not in times and "k_mega" not in times, times
        if name == "cornell":           # closed: a render takes the fused kernel, the call does not
            r.render(cams[0], opt, passes=1, readback=False)
            assert "k_bounce" in r.kernel_times()
        if name == "ajax_standin_96":   # a mesh in HBM
            assert "k_walk" in times, times
    finally:
        r.close()
    want = vr.oracle_views(name, cams, opt, 0, PASSES)
    assert planes.shape == (5, H, W, 4) and np.isfinite(want).all()
    for v in range(5):
        _same(planes[v], want[v], "%s, view %d" % (name, v))
        assert want[v][..., :3].any() and (v == 0 or not np.array_equal(want[v], want[0])), (name, v)
    if name == "veach":
        # view 4 looks straight up and sees the sky alone: a small fraction of the light of the four that see the lamps
        assert want[4][..., :3].sum()*20.0 < min(want[v][..., :3].sum() for v in range(4))


# ---------------------------------------------------------------------------
# 2: against tinsel_hip_render on a second renderer

@pytest.mark.parametrize("name", PACKS)
def test_every_plane_is_a_render_of_its_camera_at_pass_seven(name):
    cams = _cameras(name)
    scene, r, opt = _open(name)
    scene2, r2, _ = _open(name)
    try:
        planes = r.views(cams, opt, 7, PASSES)
        for v in range(5):
            _same(planes[v], _render(r2, cams[v], opt, 7, PASSES), "%s, view %d" % (name, v))
        if name == "glass":
            one = r.views(cams[3:4], opt, 7, PASSES)                # V = 1
            assert one.shape == (1, H, W, 4)
            _same(one[0], planes[3], "glass, one view")
    finally:
        r.close()
        r2.close()


# ---------------------------------------------------------------------------
# 3, 4: filters and a clamp that bites; both accumulate arms

@pytest.mark.parametrize("kind", sorted(FILTERS))
def test_filters_and_the_clamp_in_both_accumulate_arms(kind):
    cams = _cameras("veach")
    scene, r, opt = _open("veach")
    opt = FILTERS[kind](opt)
    assert opt.clamp == 4.0 and _support(opt) == (kind in ("own", "support"))
    try:
        planes = r.views(cams, opt, 0, PASSES)
        singly = r.views(cams, opt, 0, PASSES, singly=True)
        rendered = _render(r, cams[1], opt, 0, PASSES)
    finally:
        r.close()
    want = vr.oracle_views("veach", cams, opt, 0, PASSES)
    for v in range(5):
        _same(planes[v], want[v], "veach, %s, view %d" % (kind, v))
        _same(singly[v], want[v], "veach, %s, view %d, singly" % (kind, v))
    _same(rendered, want[1], "veach, %s, a render" % kind)
    # the clamp bites: without it the lamps' view differs
    loose = abi.Options.from_buffer_copy(bytes(opt))
    loose.clamp = float(np.finfo(np.float32).max)
    assert not np.array_equal(vr.oracle_view("veach", cams[0], loose, 0, PASSES), want[0])


@pytest.mark.parametrize("name", ["glass", "many_spheres"])
def test_singly_is_the_same_bits(name):
    cams = _cameras(name)
    scene, r, opt = _open(name)
    try:
        _same(r.views(cams, opt, 2, PASSES, singly=True), r.views(cams, opt, 2, PASSES), name)
    finally:
        r.close()


# ---------------------------------------------------------------------------
# 5: the cut shows nowhere

@pytest.mark.parametrize("name", ["cornell", "ajax_standin_96"])
def test_the_batch_cut_shows_nowhere(name):
    cams = _cameras(name)
    scene, r, opt = _open(name)
    try:
        whole = r.views(cams, opt, 0, PASSES)
        r.set_batch_paths(2*PASSES*W*H)
        assert tinsel_amd.plan_views(2*PASSES*W*H, W, H, PASSES, 5) == (2, PASSES, 3)       # two views per batch, three batches
        r.enable_kernel_timing(True)
        _same(r.views(cams, opt, 0, PASSES), whole, name + ", two views per batch")
        times = r.kernel_times()
        assert times["k_generate"][0] == 3 and times["k_accumulate"][0] == 3, times
        _same(r.views(cams, opt, 0, PASSES, singly=True), whole, name + ", two views per batch, singly")
        assert r.kernel_times()["k_accumulate"][0] == 5
        r.set_batch_paths(1024)
        assert tinsel_amd.plan_views(1024, W, H, PASSES, 5) == (1, 1, 5*PASSES)             # one pass of one view per batch
        _same(r.views(cams, opt, 0, PASSES), whole, name + ", one pass of one view per batch")
        assert r.kernel_times()["k_generate"][0] == 5*PASSES
    finally:
        r.close()
    _same(whole, vr.oracle_views(name, cams, opt, 0, PASSES), name)


# ---------------------------------------------------------------------------
# 6: add

def test_add_continues_a_call():
    cams = _cameras("veach")
    scene, r, opt = _open("veach")
    try:
        out = r.views(cams, opt, 0, 2)
        got = r.views(cams, opt, 2, 3, out=out, add=True)
        assert got is out
        _same(out, r.views(cams, opt, 0, 5), "veach, [0, 2) then [2, 5) against [0, 5)")
        _same(r.views(cams, opt, 2, 3, out=r.views(cams, opt, 0, 2, singly=True), add=True, singly=True), out, "veach, the same singly")
    finally:
        r.close()
    _same(out, vr.oracle_views("veach", cams, opt, 0, 5), "veach, five passes")


@pytest.mark.parametrize("kind", ["own", "gauss_2"])
def test_add_onto_a_negative_zero_and_a_nan(kind):
    """-0 + +0 is +0 and a NaN stays one: what AddSample makes of an accumulator that holds them, which a render from write_accum shows"""
    cams = _cameras("cornell")[:2]
    scene, r, opt = _open("cornell")
    opt = FILTERS[kind](opt)
    start = np.zeros((2, H, W, 4), np.float32)
    start[0, 5, 7] = -0.0
    start[0, 20, 33] = np.nan
    start[1, 0, 0] = (-0.0, 1.0, np.nan, -0.0)
    start[1, H - 1, W - 1] = -0.0
    start[1, 9, 9] = (0.5, 0.25, 0.125, 2.0)
    try:
        want = np.stack([_render(r, cams[v], opt, 3, PASSES, start[v]) for v in range(2)])
        for singly in (False, True):
            _same(r.views(cams, opt, 3, PASSES, out=start.copy(), add=True, singly=singly), want, "cornell, %s, singly = %s" % (kind, singly), bits=True)
    finally:
        r.close()
    assert np.isnan(want[0, 20, 33]).all() and np.isnan(want[1, 0, 0, 2]) and np.isfinite(want[1, 0, 0, :2]).all()


# ---------------------------------------------------------------------------
# 7: every pipeline setting

@pytest.mark.parametrize("name", ["cornell", "ajax_standin_96"])
def test_every_pipeline_setting_gives_the_same_bits(name):
    cams = _cameras(name)
    scene, r, opt = _open(name)
    want = vr.oracle_views(name, cams, opt, 1, PASSES)
    try:
        for what, p in PIPELINES.items():
            r.set_pipeline(p)
            _same(r.views(cams, opt, 1, PASSES), want, "%s, pipeline %s" % (name, what))
    finally:
        r.close()


# ---------------------------------------------------------------------------
# 8: the device entry

def test_the_device_entry_on_side_streams():
    import torch
    cams = _cameras("veach")
    scene, r, opt = _open("veach")
    try:
        dev = torch.device("cuda", r.device)
        a = torch.full((5, H, W, 4), 7.0, dtype=torch.float32, device=dev)
        b = torch.full((2, H, W, 4), 7.0, dtype=torch.float32, device=dev)
        s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(s1):
            assert r.views(cams, opt, 0, PASSES, out=a) is a
        with torch.cuda.stream(s2):
            r.views(cams[3:], opt, 4, PASSES, out=b)
        with torch.cuda.stream(s1):
            r.views(cams, opt, PASSES, 2, out=a, add=True)
        torch.cuda.synchronize(dev)
        a, b = a.cpu().numpy(), b.cpu().numpy()
    finally:
        r.close()
    _same(a, vr.oracle_views("veach", cams, opt, 0, PASSES + 2), "veach on a side stream, two calls")
    _same(b, vr.oracle_views("veach", cams[3:], opt, 4, PASSES), "veach on a second stream")


# ---------------------------------------------------------------------------
# 9: the frame state is left alone

def test_a_call_between_two_renders_leaves_the_frame_state_alone():
    cams = _cameras("cornell")
    scene, r, opt = _open("cornell")
    scene2, r2, _ = _open("cornell")
    try:
        cam = cams[0]
        r2.render(cam, opt, passes=2, readback=False)
        r2.render(cam, opt, passes=2, readback=False)
        r.render(cam, opt, passes=2, readback=False)
        before = (r.get_pass_index(), r.stats(), bytes(r.get_tuning()), r.read_accum())
        planes = r.views(cams, opt, 11, PASSES)
        after = (r.get_pass_index(), r.stats(), bytes(r.get_tuning()), r.read_accum())
        assert before[:3] == after[:3] and before[0] == 2
        _same(after[3], before[3], "the accumulator across the call")
        r.render(cam, opt, passes=2, readback=False)
        _same(r.read_accum(), r2.read_accum(), "render, views, render against render, render")
        assert r.get_pass_index() == 4 and r.stats() == r2.stats()
        _same(planes, vr.oracle_views("cornell", cams, opt, 11, PASSES), "cornell at pass 11")
    finally:
        r.close()
        r2.close()


def test_a_moved_scene_is_served_after_rebuild_scene():
    cams = _cameras("cornell")
    scene, r, opt = _open("cornell")
    try:
        prims = C.cast(scene.desc.primitives, C.POINTER(abi.Primitive))
        k = next(i for i in range(scene.desc.num_primitives) if prims[i].type == abi.GEOM_SPHERE)
        there = abi.Transform.from_buffer_copy(bytes(prims[k].start_transform))
        there.p.x += 0.3
        there.p.y += 0.2
        still = r.views(cams, opt, 0, PASSES)
        r.set_primitive_transform(k, there)
        out = np.full((5, H, W, 4), 7.0, np.float32)
        with pytest.raises(tinsel_amd.TinselHipError, match="rebuild_scene"):
            r.views(cams, opt, 0, PASSES, out=out)
        assert (out == 7.0).all()
        r.rebuild_scene()
        moved = r.views(cams, opt, 0, PASSES)
        for v in range(5):
            _same(moved[v], _render(r, cams[v], opt, 0, PASSES), "cornell moved, view %d" % v)
        assert not np.array_equal(moved[0], still[0])
    finally:
        r.close()


# ---------------------------------------------------------------------------
# 10: refusals

def test_every_refusal_leaves_out_untouched():
    import torch
    cams = _cameras("cornell")
    arr = (abi.Camera*5)(*cams)
    scene, r, opt = _open("cornell")
    L, h = r._L, r._h
    host = np.full((5, H, W, 4), 7.0, np.float32)
    dev = torch.full((5, H, W, 4), 7.0, dtype=torch.float32, device=torch.device("cuda", r.device))
    hp, dp = host.ctypes.data_as(C.c_void_p), C.c_void_p(dev.data_ptr())
    wide, normals = abi.Options.from_buffer_copy(bytes(opt)), abi.Options.from_buffer_copy(bytes(opt))
    wide.width += 1
    normals.mode = abi.MODE_NORMALS
    o = C.byref(opt)

    def refused(what, cameras=arr, views=5, options=o, passes=PASSES, flags=0, out=True, renderer=h):
        for entry, p in (("tinsel_hip_render_views", hp), ("tinsel_hip_render_views_device", dp)):
            args = [renderer, cameras, views, options, 0, passes, flags, p if out else None] + ([None] if entry.endswith("device") else [])
            assert getattr(L, entry)(*args) == -1, (what, entry)
            assert what in L.tinsel_hip_last_error().decode(), (what, entry, L.tinsel_hip_last_error())
        torch.cuda.synchronize()
        assert (host == 7.0).all() and bool((dev == 7.0).all()), what

    try:
        refused("null argument", renderer=None)
        refused("null argument", cameras=None)
        refused("null argument", options=None)
        refused("null argument", out=False)
        refused("num_views", views=0)
        refused("num_views", views=abi.MAX_VIEWS + 1)
        refused("passes", passes=0)
        refused("width/height", options=C.byref(wide))
        refused("TINSEL_MODE_PATHTRACE", options=C.byref(normals))
        refused("flag", flags=4)
        refused("flag", flags=abi.VIEWS_ADD | 8)
        assert L.tinsel_hip_render_views_device(h, arr, 5, o, 0, PASSES, 0, C.c_void_p(dev.data_ptr() + 4), None) == -1
        assert b"aligned" in L.tinsel_hip_last_error()
        r.set_arithmetic(abi.ARITH_FAST)
        refused("TINSEL_ARITH_FAST")
        r.set_arithmetic(abi.ARITH_EXACT)
        r.set_shard(1, 2)
        refused("sharded")
        r.set_shard(0, 1)
        # max_depth < 1 zeroes the planes; with add it leaves them untouched
        flat = abi.Options.from_buffer_copy(bytes(opt))
        flat.max_depth = 0
        for out in (host, dev):
            assert r.views(cams, flat, 0, PASSES, out=out, add=True) is out
        torch.cuda.synchronize()
        assert (host == 7.0).all() and bool((dev == 7.0).all())
        for out in (host, dev):
            r.views(cams, flat, 0, PASSES, out=out)
        torch.cuda.synchronize()
        assert not host.any() and not bool(dev.any())
        # and the renderer still serves
        _same(r.views(cams, opt, 0, PASSES), vr.oracle_views("cornell", cams, opt, 0, PASSES), "cornell after the refusals")
    finally:
        r.close()


# ---------------------------------------------------------------------------
# headless -views

def test_headless_writes_a_turntable(tmp_path):
    from tinsel_amd import headless
    path = str(tmp_path / "views.npz")
    pack = str(tmp_path / "cornell.pack")
    with open(pack, "wb") as fh:
        fh.write(vr.pack_bytes("cornell"))
    assert headless.main(["headless", "-width=%d" % W, "-height=%d" % H, "-spp=2", "-views=" + path, "-views_orbit=4", "-views_spp=%d" % PASSES,
                          "-views_center=0,1,0", pack]) == 0
    z = np.load(path)
    cam, opt = vr.frame("cornell")
    opt.max_samples = 2
    assert z["planes"].shape == (4, H, W, 4) and int(z["passes"]) == PASSES and np.array_equal(z["center"], np.float32([0, 1, 0]))
    cams = tinsel_amd.orbit_cameras(cam, (0.0, 1.0, 0.0), 4)
    table = np.array([tuple(c.position) + tuple(c.rotation) + (c.fov, c.shutter_start, c.shutter_end) for c in cams], np.float32)
    assert np.array_equal(z["cameras"], table)
    _same(z["planes"], vr.oracle_views("cornell", list(cams), opt, 0, PASSES), "headless -views")
    with pytest.raises(SystemExit):
        headless.main(["headless", "-views=" + path, pack])                 # -views_orbit goes with it

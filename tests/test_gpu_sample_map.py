"""Sample maps (tinsel_hip_render_sample_map / _device, kernels k_generate_samples and k_samples_accumulate): a per-pixel pass count in one call.

The yardstick is not under test: tests/sample_map_reference.py restates accumulate_reference.add_passes with one extra term (the generating
pixel has a sample at this level) and feeds it the oracle's own per-sample radiance; tests/test_sample_map_abi.py holds that statement to
the oracle without a GPU.  Every case renders 40 x 24 pixels (three by two accumulate tiles, both edges ragged) with counts up to 5 unless
it says otherwise; the oracle's radiance is computed once per (pack, options, pass_begin, levels), shared and left unchanged.  Everything is
np.array_equal on the raw floats: no case has a figure to report."""
import ctypes as C

import numpy as np
import pytest

import tinsel_amd
from tinsel_amd import abi
from tests import sample_map_reference as sm

pytestmark = pytest.mark.gpu

W, H, TOP = sm.W, sm.H, 5
PACKS = ["cornell", "veach", "glass", "motionblur", "features_probe", "many_spheres", "ajax_standin_96"]
PIPELINES = {"auto": abi.PIPELINE_AUTO, "wavefront": abi.PIPELINE_WAVEFRONT, "mega": abi.PIPELINE_MEGAKERNEL, "split": abi.PIPELINE_WAVEFRONT_SPLIT,
             "paired": abi.PIPELINE_WAVEFRONT_PAIRED}


def _open(name):
    scene = tinsel_amd.Scene(sm.pack_bytes(name))
    r = tinsel_amd.create_gpu_renderer(scene)
    r.init(W, H)
    cam, opt = sm.frame(name)
    return scene, r, cam, opt


def _same(got, want, what):
    assert got.dtype == np.float32 and got.shape == want.shape, what
    bad = (got != want).any(axis=-1)
    first = np.unravel_index(np.argmax(bad), bad.shape)
    assert np.array_equal(got, want), "%s: %d of %d pixels differ (first: %s, %s against %s)" % (what, int(bad.sum()), bad.size, first, got[first], want[first])


def _uniform(n):
    return np.full((H, W), n, np.uint16)


def _tall():
    """one pixel with 40 levels, the rest 0 or 1: most tiles are done after the first level, one runs to 40"""
    counts = (np.add.outer(np.arange(H), 2*np.arange(W)) % 3 == 0).astype(np.uint16)
    counts[13, 21] = 40
    return counts


def _filter(opt, kind, width, falloff=1.0, offset=None):
    out = abi.Options.from_buffer_copy(bytes(opt))
    out.filter.type, out.filter.width, out.filter.falloff = kind, width, falloff
    if offset is not None:
        out.filter.offset = offset
    return out


# the table of tests/test_gpu_views.py (veach: a finite clamp of 4 that bites)
FILTERS = {
    "own": lambda o: o,                                             # Gaussian 0.75: the compile-time window 3
    "box": lambda o: _filter(o, 0, 0.75),
    "gauss_1": lambda o: _filter(o, 1, 1.0, 1.0, 0.01),             # the compile-time window 4
    "gauss_2": lambda o: _filter(o, 1, 2.0, 0.5, 0.01),             # the run-time window
    "gauss_2_5": lambda o: _filter(o, 1, 2.5, 0.5, 0.01),           # no tiled form: refused
}


# ---------------------------------------------------------------------------
# 1: a uniform map is a render

@pytest.mark.parametrize("name", PACKS)
def test_a_uniform_map_is_the_oracles_accumulator_and_a_views_plane(name):
    scene, r, cam, opt = _open(name)
    try:
        r.enable_kernel_timing(True)
        got = r.sample_map(cam, opt, _uniform(3))
        times = r.kernel_times()
        # one generation and one accumulate launch; never the fused kernel, which makes the camera's paths itself
        assert times["k_generate"][0] == 1 and times["k_accumulate"][0] == 1 and "k_bounce" not in times and "k_mega" not in times, times
        if name == "ajax_standin_96":   # a mesh in HBM
            assert "k_walk" in times, times
        plane = r.views([cam], opt, 0, 3)[0]
    finally:
        r.close()
    want = sm.oracle_levels(name, cam, opt, 0, 3)[0]
    assert np.isfinite(want).all() and want[..., :3].any()
    _same(got, want, name + " against the oracle")
    _same(got, plane, name + " against views([camera])")


# ---------------------------------------------------------------------------
# 2: a random map -- the test that cannot pass without the feature

@pytest.mark.parametrize("name", ["cornell", "veach", "motionblur", "ajax_standin_96"])
def test_a_random_map_is_the_masked_statement(name):
    counts = sm.random_counts(11)
    assert (counts == 0).any() and (counts == TOP).any() and counts.max() == TOP
    scene, r, cam, opt = _open(name)
    try:
        got = r.sample_map(cam, opt, counts)
        full = r.sample_map(cam, opt, _uniform(TOP))
    finally:
        r.close()
    _same(got, sm.statement(name, cam, opt, 0, counts), name + ", a random map")
    _same(full, sm.oracle_levels(name, cam, opt, 0, TOP)[0], name + ", uniform 5")
    assert not np.array_equal(got, full) and np.isfinite(got).all()
    assert (got[..., 3] <= full[..., 3]).all()          # a missing sample is skipped, not added as black: the weight does not see it


# ---------------------------------------------------------------------------
# 3: a crop

@pytest.mark.parametrize("name", ["cornell", "motionblur"])
def test_a_crop_across_tile_boundaries(name):
    x0, y0, x1, y1 = 5, 3, 27, 19
    counts = tinsel_amd.crop_sample_map(W, H, x0, y0, x1, y1, 4)
    scene, r, cam, opt = _open(name)
    try:
        got = r.sample_map(cam, opt, counts)
    finally:
        r.close()
    _same(got, sm.statement(name, cam, opt, 0, counts), name + ", a crop")
    # a sample lands within [int(x - fw), int(x + fw)] of its raster position x in [i, i + 1): pixel p hears of the generating pixels
    # p - 1 - floor(fw) .. p + ceil(fw) and of no other
    fw = opt.filter.width
    lo, hi = 1 + int(np.floor(fw)), int(np.ceil(fw))
    ii, jj = np.meshgrid(np.arange(W), np.arange(H))
    near = (ii + hi >= x0) & (ii - lo < x1) & (jj + hi >= y0) & (jj - lo < y1)
    assert (~near).sum() > 200 and not got[~near].any(), "pixels beyond the filter's reach must stay exactly zero"
    # inside, away from the rim, the crop IS the full frame
    full = sm.oracle_levels(name, cam, opt, 0, 4)[0]
    inner = (slice(y0 + lo, y1 - hi), slice(x0 + lo, x1 - hi))          # pixels all of whose generating pixels are in the rectangle
    assert full[inner][..., 3].all()
    _same(got[inner], full[inner], name + ", the crop's interior against the full frame")


# ---------------------------------------------------------------------------
# 4: one tall pixel

@pytest.mark.parametrize("name", ["cornell", "ajax_standin_96"])
def test_one_tall_pixel(name):
    counts = _tall()
    assert counts.max() == 40 and set(np.unique(counts)) == {0, 1, 40}
    scene, r, cam, opt = _open(name)
    try:
        got = r.sample_map(cam, opt, counts)
    finally:
        r.close()
    _same(got, sm.statement(name, cam, opt, 0, counts), name + ", one pixel of 40 levels")
    top = np.unravel_index(np.argmax(got[..., 3]), (H, W))
    assert top[0] in (13, 14) and top[1] in (21, 22), top           # the 40 samples land on their pixel and the one below / right of it


# ---------------------------------------------------------------------------
# 5: filters, and a clamp that bites

@pytest.mark.parametrize("kind", ["own", "box", "gauss_1", "gauss_2"])
def test_filters_and_the_clamp(kind):
    counts = sm.random_counts(23)
    scene, r, cam, opt = _open("veach")
    opt = FILTERS[kind](opt)
    assert opt.clamp == 4.0
    try:
        got = r.sample_map(cam, opt, counts)
    finally:
        r.close()
    want = sm.statement("veach", cam, opt, 0, counts)
    _same(got, want, "veach, " + kind)
    loose = abi.Options.from_buffer_copy(bytes(opt))
    loose.clamp = float(np.finfo(np.float32).max)
    assert not np.array_equal(sm.statement("veach", cam, loose, 0, counts), want)      # the clamp bites


def test_a_filter_wider_than_the_tiles_hold_is_refused():
    import torch
    scene, r, cam, opt = _open("veach")
    opt = FILTERS["gauss_2_5"](opt)
    try:
        host = np.full((H, W, 4), 7.0, np.float32)
        dev = torch.full((H, W, 4), 7.0, dtype=torch.float32, device=torch.device("cuda", r.device))
        for out in (host, dev):
            with pytest.raises(tinsel_amd.TinselHipError, match="no untiled masked accumulate"):
                r.sample_map(cam, opt, _uniform(2), out=out)
        torch.cuda.synchronize()
        assert (host == 7.0).all() and bool((dev == 7.0).all())
        assert r.views([cam], opt, 0, 2).any()              # views take it: one untiled k_accumulate per view
    finally:
        r.close()


# ---------------------------------------------------------------------------
# 6: every pipeline setting

@pytest.mark.parametrize("name", ["cornell", "ajax_standin_96"])
def test_every_pipeline_setting_gives_the_same_bits(name):
    counts = sm.random_counts(5)
    scene, r, cam, opt = _open(name)
    want = sm.statement(name, cam, opt, 1, counts)
    try:
        for what, p in PIPELINES.items():
            r.set_pipeline(p)
            _same(r.sample_map(cam, opt, counts, pass_begin=1), want, "%s, pipeline %s" % (name, what))
    finally:
        r.close()


# ---------------------------------------------------------------------------
# 7: the cut shows nowhere

@pytest.mark.parametrize("name", ["cornell", "ajax_standin_96"])
def test_the_batch_cut_shows_nowhere(name):
    scene, r, cam, opt = _open(name)
    maps = {"random": sm.random_counts(17), "tall": _tall()}
    try:
        whole = {k: r.sample_map(cam, opt, c) for k, c in maps.items()}
        r.enable_kernel_timing(True)
        r.set_batch_paths(1024)                             # below one level of 960 pixels twice over: one level per batch
        for k, c in maps.items():
            levels, batches, paths, most = tinsel_amd.plan_sample_map(1024, W, H, c)
            assert (levels, batches, paths, most) == (1, int(c.max()), int(c.sum()), int(c.max()))
            _same(r.sample_map(cam, opt, c), whole[k], "%s, %s, one level per batch" % (name, k))
            times = r.kernel_times()
            assert times["k_generate"][0] == batches and times["k_accumulate"][0] == batches, times
        r.set_batch_paths(2*W*H + 100)                      # two levels per batch, a ragged last batch
        assert tinsel_amd.plan_sample_map(2*W*H + 100, W, H, maps["random"])[:2] == (2, 3)
        _same(r.sample_map(cam, opt, maps["random"]), whole["random"], name + ", two levels per batch")
        assert r.kernel_times()["k_generate"][0] == 3
    finally:
        r.close()
    # (the tall map's batches 1 .. 39 hold one path each)
    assert [int(sm.batch_offsets(maps["tall"], t, 1)[-1]) for t in (0, 1, 39)] == [int((maps["tall"] > 0).sum()), 1, 1]
    for k, c in maps.items():
        _same(whole[k], sm.statement(name, cam, opt, 0, c), "%s, %s" % (name, k))


# ---------------------------------------------------------------------------
# 8: add

def test_add_continues_a_call():
    a, begin = 2, 3
    c = sm.random_counts(29, top=3)
    scene, r, cam, opt = _open("veach")
    try:
        out = r.sample_map(cam, opt, _uniform(a), pass_begin=begin)
        _same(out, r.views([cam], opt, begin, a)[0], "veach, a uniform call of two passes")
        got = r.sample_map(cam, opt, c, pass_begin=begin + a, out=out, add=True)
        assert got is out
        _same(out, r.sample_map(cam, opt, (a + c).astype(np.uint16), pass_begin=begin), "veach, uniform 2 then a map on top against the single map")
        # a render's accumulator continues the same way
        r.write_accum(np.zeros((H, W, 4), np.float32), begin)
        r.render(cam, opt, passes=a, readback=False)
        _same(r.sample_map(cam, opt, c, pass_begin=begin + a, out=r.read_accum(), add=True), out, "veach, a render of two passes then a map on top")
    finally:
        r.close()
    _same(out, sm.statement("veach", cam, opt, begin, a + c), "veach, the single map against the statement")


def test_a_map_of_zeros_and_a_depth_of_zero():
    import torch
    scene, r, cam, opt = _open("cornell")
    flat = abi.Options.from_buffer_copy(bytes(opt))
    flat.max_depth = 0
    try:
        host = np.full((H, W, 4), 7.0, np.float32)
        dev = torch.full((H, W, 4), 7.0, dtype=torch.float32, device=torch.device("cuda", r.device))
        r.enable_kernel_timing(True)
        for o, counts in ((opt, _uniform(0)), (flat, _uniform(3))):
            for out in (host, dev):
                assert r.sample_map(cam, o, counts, out=out, add=True) is out
            torch.cuda.synchronize()
            assert (host == 7.0).all() and bool((dev == 7.0).all())
        for o, counts in ((opt, _uniform(0)), (flat, _uniform(3))):
            host[:] = 7.0
            dev.fill_(7.0)
            for out in (host, dev):
                r.sample_map(cam, o, counts, out=out)
                assert "k_generate" not in r.kernel_times()         # nothing is launched
            torch.cuda.synchronize()
            assert not host.any() and not bool(dev.any())
        # and the renderer still serves
        _same(r.sample_map(cam, opt, _uniform(2)), sm.oracle_levels("cornell", cam, opt, 0, 2)[0], "cornell after the empty calls")
    finally:
        r.close()


# ---------------------------------------------------------------------------
# 9: the frame state is left alone

def test_a_call_between_two_renders_leaves_the_frame_state_alone():
    counts = sm.random_counts(31)
    scene, r, cam, opt = _open("cornell")
    scene2, r2, _, _ = _open("cornell")
    try:
        r2.render(cam, opt, passes=2, readback=False)
        r2.render(cam, opt, passes=2, readback=False)
        r.render(cam, opt, passes=2, readback=False)
        before = (r.get_pass_index(), r.stats(), bytes(r.get_tuning()), r.read_accum())
        got = r.sample_map(cam, opt, counts, pass_begin=11)
        after = (r.get_pass_index(), r.stats(), bytes(r.get_tuning()), r.read_accum())
        assert before[:3] == after[:3] and before[0] == 2
        _same(after[3], before[3], "the accumulator across the call")
        r.render(cam, opt, passes=2, readback=False)
        _same(r.read_accum(), r2.read_accum(), "render, sample map, render against render, render")
        assert r.get_pass_index() == 4 and r.stats() == r2.stats()
        _same(got, sm.statement("cornell", cam, opt, 11, counts), "cornell at pass 11")
    finally:
        r.close()
        r2.close()


# ---------------------------------------------------------------------------
# 10: the device entry

def test_the_device_entry_on_a_side_stream_at_pass_seven():
    import torch
    counts, more = sm.random_counts(37), sm.random_counts(41, top=2)
    scene, r, cam, opt = _open("veach")
    try:
        dev = torch.device("cuda", r.device)
        a = torch.full((H, W, 4), 7.0, dtype=torch.float32, device=dev)
        side = torch.cuda.Stream(dev)
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(side):
            assert r.sample_map(cam, opt, counts, pass_begin=7, out=a) is a
            r.sample_map(cam, opt, more, pass_begin=7 + TOP, out=a, add=True)
        assert a.is_cuda
        torch.cuda.synchronize(dev)
        a = a.cpu().numpy()
    finally:
        r.close()
    want = sm.statement("veach", cam, opt, 7, counts)
    _same(a, sm.statement("veach", cam, opt, 7 + TOP, more, start=want), "veach on a side stream, two calls")


# ---------------------------------------------------------------------------
# 11: refusals

def test_every_refusal_leaves_out_untouched():
    import torch
    scene, r, cam, opt = _open("cornell")
    L, h = r._L, r._h
    counts = sm.random_counts(43)
    host = np.full((H, W, 4), 7.0, np.float32)
    dev = torch.full((H, W, 4), 7.0, dtype=torch.float32, device=torch.device("cuda", r.device))
    hp, dp, cp = host.ctypes.data_as(C.c_void_p), C.c_void_p(dev.data_ptr()), counts.ctypes.data_as(C.c_void_p)
    wide, normals = abi.Options.from_buffer_copy(bytes(opt)), abi.Options.from_buffer_copy(bytes(opt))
    wide.width += 1
    normals.mode = abi.MODE_NORMALS
    o, c = C.byref(opt), C.byref(cam)

    def refused(what, camera=c, options=o, cnt=cp, flags=0, out=True, renderer=h):
        for entry, p in (("tinsel_hip_render_sample_map", hp), ("tinsel_hip_render_sample_map_device", dp)):
            args = [renderer, camera, options, 0, cnt, flags, p if out else None] + ([None] if entry.endswith("device") else [])
            assert getattr(L, entry)(*args) == -1, (what, entry)
            assert what in L.tinsel_hip_last_error().decode(), (what, entry, L.tinsel_hip_last_error())
        torch.cuda.synchronize()
        assert (host == 7.0).all() and bool((dev == 7.0).all()), what

    try:
        refused("null argument", renderer=None)
        refused("null argument", camera=None)
        refused("null argument", options=None)
        refused("null argument", cnt=None)
        refused("null argument", out=False)
        refused("width/height", options=C.byref(wide))
        refused("TINSEL_MODE_PATHTRACE", options=C.byref(normals))
        refused("flag", flags=2)
        refused("flag", flags=abi.SAMPLES_ADD | 8)
        assert L.tinsel_hip_render_sample_map_device(h, c, o, 0, cp, 0, C.c_void_p(dev.data_ptr() + 4), None) == -1
        assert b"aligned" in L.tinsel_hip_last_error()
        r.set_arithmetic(abi.ARITH_FAST)
        refused("TINSEL_ARITH_FAST")
        r.set_arithmetic(abi.ARITH_EXACT)
        r.set_shard(1, 2)
        refused("sharded")
        r.set_shard(0, 1)
        # a moved primitive without a rebuild
        prims = C.cast(scene.desc.primitives, C.POINTER(abi.Primitive))
        k = next(i for i in range(scene.desc.num_primitives) if prims[i].type == abi.GEOM_SPHERE)
        there = abi.Transform.from_buffer_copy(bytes(prims[k].start_transform))
        there.p.x += 0.3
        there.p.y += 0.2
        still = r.sample_map(cam, opt, counts)
        r.set_primitive_transform(k, there)
        refused("rebuild_scene")
        r.rebuild_scene()
        moved = r.sample_map(cam, opt, counts)
        assert not np.array_equal(moved, still)
        r.write_accum(np.zeros((H, W, 4), np.float32), 0)
        r.render(cam, opt, passes=TOP, readback=False)
        _same(r.sample_map(cam, opt, _uniform(TOP)), r.read_accum(), "cornell moved, uniform 5 against a render")
    finally:
        r.close()
    _same(still, sm.statement("cornell", cam, opt, 0, counts), "cornell before the move")


# ---------------------------------------------------------------------------
# headless -samplemap

def test_headless_writes_the_plane_and_the_counts(tmp_path):
    from tinsel_amd import headless
    counts = sm.random_counts(47)
    src, path, pack = str(tmp_path / "counts.npy"), str(tmp_path / "plane.npz"), str(tmp_path / "cornell.pack")
    np.save(src, counts)
    with open(pack, "wb") as fh:
        fh.write(sm.pack_bytes("cornell"))
    assert headless.main(["headless", "-width=%d" % W, "-height=%d" % H, "-spp=2", "-samplemap=" + src, "-samplemap_out=" + path,
                          "-samplemap_begin=3", pack]) == 0
    z = np.load(path)
    cam, opt = sm.frame("cornell")
    opt.max_samples = 2
    assert z["plane"].shape == (H, W, 4) and int(z["pass_begin"]) == 3 and np.array_equal(z["counts"], counts) and z["counts"].dtype == np.uint16
    _same(z["plane"], sm.statement("cornell", cam, opt, 3, counts), "headless -samplemap")
    with pytest.raises(SystemExit):
        headless.main(["headless", "-samplemap=" + src, pack])                 # -samplemap_out goes with it

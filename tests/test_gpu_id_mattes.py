"""ID mattes (tinsel_hip_render_id_mattes / _device; kernels k_ids, k_ids_accumulate, k_ids_rank): per pixel the ranked list of (primitive id,
filter-weight sum) pairs on the beauty's own samples, bit for bit.

The expected value comes from code that is not under test.  For the path of pixel (i, j) in pass s the camera record is the one
tests/test_gpu_radiance_query.py::_starts builds from the reference alone; its id is the primitive of HipRenderer.trace_rays(..., "closest")
-- k_query, pinned to the reference's Trace() by tests/test_gpu_ray_query.py -- or -1.  The lists are tests/id_mattes_reference.id_mattes of
those ids: the header's rule as sequential numpy float32, which tests/test_id_mattes_abi.py holds to accumulate_reference.add_passes; where
nothing overflows the weights are also compared with add_passes of every id's indicator directly.  Comparisons are on the uint32 view of
every word of every plane.

The frame is 50 x 37 with 3 passes unless stated: no multiple of 64, ragged accumulate tiles, several workgroups."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import tinsel_amd
from tinsel_amd import abi, headless
from tests import oracle_api as oa
from tests.accumulate_reference import add_passes, constructor_offset
from tests.id_mattes_reference import id_mattes
from tests.test_gpu_radiance_query import _frame, _starts
from tests.test_gpu_ray_query import _cam_opt, _renderer

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not oa.have_ref(), reason="oracle/_ref not built")]

W, H, PASSES = 50, 37, 3
E, M = abi.ID_EMPTY, abi.ID_MISS
# (cornell_probe is closed by unbounded planes -- no camera path leaves it, from any camera -- so the miss that holds a slot is asserted on
# fuzz:01, a third of whose paths leave the scene and which does not overflow eight slots)
PARITY_SCENES = ["cornell", "glass", "motionblur", "cornell_probe", "ajax_standin_96", "mesh:beyond_flat:1", "fuzz:01"]
OVERFLOW_SCENES = ["many_spheres", "fuzz:00"]
G = abi.FILTER_GAUSSIAN
FILTERS = {
    "box_1.0": (abi.FILTER_BOX, 1.0, 1.0, constructor_offset(1.0, 1.0)),
    "gauss_0.75": (G, 0.75, 1.0, constructor_offset(0.75, 1.0)),
    "gauss_1.0_loader": (G, 1.0, 1.0, constructor_offset(0.75, 1.0)),        # the loader keeps Filter(gaussian, 0.75, 1.0)'s offset: zero weights by construction
    "gauss_1.5": (G, 1.5, 1.0, constructor_offset(1.5, 1.0)),                # the tiled form's run-time window
    "gauss_2.5": (G, 2.5, 1.0, constructor_offset(2.5, 1.0)),                # the generic form
}
KEYS = ("ids", "weights", "residual", "total")


def _bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype in (np.float32, np.int32), a.dtype
    return a.view(np.uint32)


def _same(got, want, what):
    for k in KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype == (np.int32 if k == "ids" else np.float32) and g.shape == w.shape, (what, k, g.dtype, g.shape, w.shape)
        bad = _bits(g) != _bits(w)
        assert not bad.any(), "%s, %s: %d of %d words differ (first at %s: %s against %s)" % (
            what, k, int(bad.sum()), bad.size, np.unravel_index(np.argmax(bad), bad.shape), g[np.unravel_index(np.argmax(bad), bad.shape)],
            w[np.unravel_index(np.argmax(bad), bad.shape)])


def _path_ids(r, starts, width=W, height=H):
    """[passes, height, width] int32: the closest-hit primitive of every path, -1 where it leaves the scene, from trace_rays on renderer r"""
    rays = np.zeros((len(starts), 8), np.float32)
    for k, f in enumerate(("ox", "oy", "oz", "time", "dx", "dy", "dz")):
        rays[:, k] = starts[f]
    rays[:, 7] = np.inf
    prim = np.asarray(r.trace_rays(rays, "closest")["primitive"]).astype(np.int32)
    assert prim.min() >= M
    return np.ascontiguousarray(prim.reshape(-1, height, width))


def _filter_of(opt):
    return (opt.filter.type, opt.filter.width, opt.filter.falloff, opt.filter.offset)


@functools.lru_cache(maxsize=None)
def _case(name, pass_begin=0, passes=PASSES, fast=False):
    """(the id of every path, the passes' seeds, the pack's own filter) of a scene's own camera at 50 x 37: computed once, shared, left unchanged"""
    R = oa.RefOracle()
    scene, r = _renderer(name)
    try:
        cam, opt = _cam_opt(scene)
        starts = _starts(R, cam, W, H, pass_begin + passes)[pass_begin*W*H:]
        if fast:
            r.set_arithmetic(abi.ARITH_FAST)
        ids = _path_ids(r, starts)
    finally:
        r.close()
    ids.setflags(write=False)
    return ids, tuple(int(R.pass_seed(pass_begin + s)) for s in range(passes)), tuple(_filter_of(opt))


def _owned(rank, world, tile):
    j, i = np.mgrid[0:H, 0:W]
    tiles_x = (W + tile - 1)//tile
    return ((j//tile)*tiles_x + i//tile) % world == rank


@functools.lru_cache(maxsize=None)
def _want(name, filt=None, slots=8, pass_begin=0, passes=PASSES, fast=False, shard=None):
    """the statement's lists for a case; filt: a key of FILTERS, None = the pack's own; shard = (rank, world, tile)"""
    ids, seeds, own = _case(name, pass_begin, passes, fast)
    out = id_mattes(ids, seeds, FILTERS[filt] if filt else own, slots, owned=_owned(*shard) if shard else None)
    for a in out.values():
        a.setflags(write=False)
    return out


def _open(name):
    scene, r = _renderer(name)
    cam, opt = _cam_opt(scene)
    opt = _frame(opt, W, H)
    r.init(W, H)
    return scene, r, cam, opt


def _with_filter(opt, filt):
    o = opt.copy()
    o.filter.type, o.filter.width, o.filter.falloff, o.filter.offset = int(filt[0]), float(filt[1]), float(filt[2]), float(filt[3])
    return o


# ---------------------------------------------------------------------------
# 1: parity per scene, eight slots, the pack's own filter

@pytest.mark.parametrize("name", PARITY_SCENES)
def test_the_lists_are_the_first_hits_gathered_as_the_beauty_is(name):
    ids, seeds, filt = _case(name)
    want = _want(name)
    assert (W*H*PASSES) % 64 != 0
    assert not want["residual"].any(), "%s overflows eight slots" % name
    assert ((want["ids"] != E).sum(axis=0) >= 2).any()
    if name == "fuzz:01":
        assert (want["ids"] == M).any() and (want["ids"][0] == M).any() and (want["ids"][1:] == M).any()       # the miss holds a slot, first and later ones
    if name == "motionblur":
        assert len(np.unique(ids)) <= 6             # at most five primitives and the miss: it cannot overflow by count
    scene, r, cam, opt = _open(name)
    try:
        got = r.id_mattes(cam, opt, 0, PASSES, 8)
    finally:
        r.close()
    assert list(got) == list(KEYS)
    _same(got, want, name)
    # nothing overflows: every id's weight is AddSample's sum of its indicator, and the total AddSample's weight
    values, counts = np.unique(ids, return_counts=True)
    for v in values[np.argsort(-counts, kind="stable")][:12]:          # (the twelve most frequent where a scene has more: seconds, not minutes)
        radiance = np.zeros((PASSES, H, W, 4), np.float32)
        radiance[..., 0] = ids == v
        plane = add_passes(np.zeros((H, W, 4), np.float32), radiance, seeds, filt, np.inf)
        mine = np.where(got["ids"] == v, got["weights"], np.float32(0)).sum(axis=0, dtype=np.float32)
        assert np.array_equal(_bits(mine), _bits(plane[..., 0])), (name, int(v))
        assert np.array_equal(_bits(got["total"]), _bits(plane[..., 3])), name


# ---------------------------------------------------------------------------
# 2: more ids than slots

@pytest.mark.parametrize("slots", [1, 2])
@pytest.mark.parametrize("name", OVERFLOW_SCENES)
def test_what_finds_no_slot_goes_to_the_residual(name, slots):
    want = _want(name, None, slots)
    assert want["residual"].any(), "%s does not overflow %d slots" % (name, slots)
    assert want["ids"].shape == (slots, H, W)
    scene, r, cam, opt = _open(name)
    try:
        got = r.id_mattes(cam, opt, 0, PASSES, slots)
    finally:
        r.close()
    _same(got, want, "%s, %d slots" % (name, slots))


# ---------------------------------------------------------------------------
# 3: filters -- the tiled form's three windows, zero weights, the generic form

@pytest.mark.parametrize("slots", [8, 2])
@pytest.mark.parametrize("filt", sorted(FILTERS))
def test_every_filter_gives_the_statements_lists(filt, slots):
    want = _want("cornell", filt, slots)
    if slots == 2:
        assert want["residual"].any()
    scene, r, cam, opt = _open("cornell")
    try:
        got = r.id_mattes(cam, _with_filter(opt, FILTERS[filt]), 0, PASSES, slots)
    finally:
        r.close()
    _same(got, want, "%s, %d slots" % (filt, slots))


# ---------------------------------------------------------------------------
# 4: pass_begin and the batch cut

@pytest.mark.parametrize("filt", [None, "gauss_2.5"])
def test_the_batch_cut_shows_nowhere(filt):
    want = _want("cornell", filt, 3, 2, PASSES)
    scene, r, cam, opt = _open("cornell")
    if filt:
        opt = _with_filter(opt, FILTERS[filt])
    try:
        r.enable_kernel_timing(True)
        one = r.id_mattes(cam, opt, 2, PASSES, 3)
        t1 = r.kernel_times()
        r.set_batch_paths(1024)                 # the smallest the library takes: a pass (1850 slots) per batch
        cut = r.id_mattes(cam, opt, 2, PASSES, 3)
        t3 = r.kernel_times()
    finally:
        r.close()
    # k_ids is timed as k_features; the gather and the ranking have no class
    assert sorted(t1) == sorted(t3) == ["k_features"] and t1["k_features"][0] == 1 and t3["k_features"][0] == PASSES >= 2
    _same(one, want, "one batch")
    _same(cut, one, "three batches")
    assert want["residual"].any()


# ---------------------------------------------------------------------------
# 5: the total plane is the accumulator's weight

@pytest.mark.parametrize("name", ["cornell", "motionblur"])
def test_the_total_is_the_w_of_the_depth_plane(name):
    scene, r, cam, opt = _open(name)
    try:
        got = r.id_mattes(cam, opt, 0, PASSES, 6)
        depth = r.features(cam, opt, 0, PASSES, which=("depth",))["depth"]
    finally:
        r.close()
    assert np.array_equal(_bits(got["total"]), _bits(depth[..., 3])) and got["total"].min() > 0
    _same(got, _want(name, None, 6), name)


# ---------------------------------------------------------------------------
# 6: what the call leaves alone

@pytest.mark.parametrize("lookahead", [0, 1])
def test_a_call_between_two_renders_changes_nothing(lookahead):
    scene, r, cam, opt = _open("cornell")
    try:
        r.set_lookahead(lookahead)
        r.render(cam, opt, passes=2)
        plain = r.render(cam, opt, passes=2).copy()
        r.init(W, H)
        r.set_pass_index(0)
        r.render(cam, opt, passes=2)
        before = (r.get_pass_index(), r.stats(), r.get_tuning().as_dict())
        got = r.id_mattes(cam, opt, 0, PASSES, 8)
        assert (r.get_pass_index(), r.stats(), r.get_tuning().as_dict()) == before and before[0] == 2
        between = r.render(cam, opt, passes=2)
    finally:
        r.close()
    assert np.array_equal(between, plain) and between.tobytes() == plain.tobytes()
    _same(got, _want("cornell"), "between two renders")


# ---------------------------------------------------------------------------
# 7: the device entry

def test_the_device_entry_on_a_side_stream():
    torch = pytest.importorskip("torch")
    scene, r, cam, opt = _open("ajax_standin_96")
    try:
        host = r.id_mattes(cam, opt, 0, PASSES, 5)
        ids = torch.full((6, H, W), 9, dtype=torch.int32, device="cuda")
        weights = torch.full((8, H, W), 9.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            got = r.id_mattes(cam, opt, 0, PASSES, 5, out=(ids[:5], weights[:7]))
        beauty = r.render(cam, opt, passes=1)         # enqueued right behind it on the renderer's own stream: no synchronise in between
        side.synchronize()
        assert all(got[k].is_cuda for k in KEYS)
        _same({k: got[k].cpu().numpy() for k in KEYS}, host, "device entry")
        assert (ids[5].cpu().numpy() == 9).all() and (weights[7].cpu().numpy() == 9.0).all() and np.isfinite(beauty).all()
        # another call with other slots on another stream right behind it: the later call waits for the earlier one's buffers
        other = torch.cuda.Stream()
        ids2 = torch.full((2, H, W), 9, dtype=torch.int32, device="cuda")
        weights2 = torch.full((4, H, W), 9.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            first = r.id_mattes(cam, opt, 0, PASSES, 5, out=(ids[:5], weights[:7]))
        with torch.cuda.stream(other):
            second = r.id_mattes(cam, opt, 0, PASSES, 2, out=(ids2, weights2))
        torch.cuda.synchronize()
        _same({k: first[k].cpu().numpy() for k in KEYS}, host, "first stream")
        _same({k: second[k].cpu().numpy() for k in KEYS}, _want("ajax_standin_96", None, 2), "second stream")
    finally:
        r.close()
    _same(host, _want("ajax_standin_96", None, 5), "ajax_standin_96")


def test_refusals_write_nothing():
    torch = pytest.importorskip("torch")
    scene, r, cam, opt = _open("cornell")
    fresh_scene, fresh = _renderer("cornell")           # never init-ed
    L, hnd = r._L, r._h
    ids, weights = np.full((6, H, W), 5, np.int32), np.full((8, H, W), 5.0, np.float32)
    ip, wp = ids.ctypes.data_as(C.c_void_p), weights.ctypes.data_as(C.c_void_p)
    dids = torch.full((6*H*W + 8,), 5, dtype=torch.int32, device="cuda")
    dweights = torch.full((8*H*W + 8,), 5.0, dtype=torch.float32, device="cuda")
    normals, wrong = opt.copy(), opt.copy()
    normals.mode = abi.MODE_NORMALS
    wrong.width = W + 1
    cp, opp = C.byref(cam), C.byref(opt)

    def untouched():
        torch.cuda.synchronize()
        return (ids == 5).all() and (weights == 5.0).all() and (dids.cpu().numpy() == 5).all() and (dweights.cpu().numpy() == 5.0).all()

    try:
        cases = [
            ("null", (None, cp, opp, 0, PASSES, 6, ip, wp)),
            ("null", (hnd, cp, opp, 0, PASSES, 6, None, wp)),
            ("null", (hnd, cp, opp, 0, PASSES, 6, ip, None)),
            ("passes", (hnd, cp, opp, 0, 0, 6, ip, wp)),
            ("slots", (hnd, cp, opp, 0, PASSES, 0, ip, wp)),
            ("slots", (hnd, cp, opp, 0, PASSES, 9, ip, wp)),
            ("mode", (hnd, cp, C.byref(normals), 0, PASSES, 6, ip, wp)),
            ("width/height", (hnd, cp, C.byref(wrong), 0, PASSES, 6, ip, wp)),           # a size that is not the last init's
            ("width/height", (fresh._h, cp, opp, 0, PASSES, 6, ip, wp)),
        ]
        for cause, args in cases:
            assert L.tinsel_hip_init(None, 0, 0) == -1 and L.tinsel_hip_last_error().startswith(b"init:")      # another entry's text in between
            assert L.tinsel_hip_render_id_mattes(*args) == -1, (cause, args)
            msg = L.tinsel_hip_last_error()
            assert msg.startswith(b"render_id_mattes:") and cause.encode() in msg, msg
            dargs = args[:6] + (dids.data_ptr() if args[6] is not None else None, dweights.data_ptr() if args[7] is not None else None, None)
            assert L.tinsel_hip_render_id_mattes_device(*dargs) == -1, (cause, dargs)
            msg = L.tinsel_hip_last_error()
            assert msg.startswith(b"render_id_mattes_device:") and cause.encode() in msg, msg
            assert untouched()
        # the device entry's own: a pointer that is not 16-byte aligned, either of the two
        for a, b in ((dids.data_ptr() + 4, dweights.data_ptr()), (dids.data_ptr(), dweights.data_ptr() + 8)):
            assert L.tinsel_hip_render_id_mattes_device(hnd, cp, opp, 0, PASSES, 6, a, b, None) == -1
            msg = L.tinsel_hip_last_error()
            assert msg.startswith(b"render_id_mattes_device:") and b"16-byte aligned" in msg
        assert untouched()
        # a moved primitive without the rebuild, both entries
        last = scene.num_primitives - 1
        t = abi.Transform.from_buffer_copy(bytes(C.cast(scene.desc.primitives, C.POINTER(abi.Primitive))[last].start_transform))
        t.p.x += 0.25
        r.set_primitive_transform(last, t, t)
        assert L.tinsel_hip_render_id_mattes(hnd, cp, opp, 0, PASSES, 6, ip, wp) == -1
        msg = L.tinsel_hip_last_error()
        assert msg.startswith(b"render_id_mattes:") and b"call tinsel_hip_rebuild_scene first" in msg
        assert L.tinsel_hip_render_id_mattes_device(hnd, cp, opp, 0, PASSES, 6, dids.data_ptr(), dweights.data_ptr(), None) == -1
        assert L.tinsel_hip_last_error().startswith(b"render_id_mattes_device:") and untouched()
        r.rebuild_scene()
        assert L.tinsel_hip_render_id_mattes(hnd, cp, opp, 0, PASSES, 6, ip, wp) == 0 and not (ids == 5).all() and not (weights == 5.0).all()
    finally:
        r.close()
        fresh.close()


# ---------------------------------------------------------------------------
# 8: shards

@pytest.mark.parametrize("filt", [None, "gauss_2.5"])
def test_a_shard_gives_its_partial_list_and_the_merge_the_frames(filt):
    tile, world, slots = 16, 2, 8
    scene, r, cam, opt = _open("cornell")
    if filt:
        opt = _with_filter(opt, FILTERS[filt])
    try:
        whole = r.id_mattes(cam, opt, 0, PASSES, slots)
        parts = []
        for rank in range(world):
            r.set_shard(rank, world, tile)
            parts.append(r.id_mattes(cam, opt, 0, PASSES, slots))
    finally:
        r.close()
    _same(whole, _want("cornell", filt, slots), "the whole frame")
    assert not whole["residual"].any()
    for rank in range(world):
        _same(parts[rank], _want("cornell", filt, slots, shard=(rank, world, tile)), "rank %d of %d" % (rank, world))
    assert all(p["total"].any() and not np.array_equal(p["total"], whole["total"]) for p in parts)
    merged = tinsel_amd.merge_id_mattes(parts, slots)
    # the same ids under every pixel
    assert np.array_equal(np.sort(merged["ids"], axis=0), np.sort(whole["ids"], axis=0))
    # n non-negative fp32 terms summed in two orders differ by at most 2 (n - 1) 2^-24 times their sum (each partial sum is at most
    # the total and rounds by at most 2^-24 of it; n - 1 adds either way).  n: the candidates a pixel can have
    fw = FILTERS[filt][1] if filt else _case("cornell")[2][1]
    window = 1 + int(np.floor(fw)) + int(np.ceil(fw)) + 1
    n = PASSES*window*window
    bound = 2.0*(n - 1)*2.0**-24*whole["total"].astype(np.float64)
    worst = 0.0
    for k in range(slots):
        theirs = np.where(whole["ids"] == merged["ids"][k][None], whole["weights"], np.float32(0)).sum(axis=0, dtype=np.float64)
        err = np.abs(merged["weights"][k].astype(np.float64) - theirs)
        worst = max(worst, float((err/np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (k, float(err.max()))
    for k in ("residual", "total"):
        assert (np.abs(merged[k].astype(np.float64) - whole[k].astype(np.float64)) <= bound).all(), k
    print("merge against the unsharded lists: largest error %.3g of the bound (n = %d)" % (worst, n))


# ---------------------------------------------------------------------------
# 9: the tolerance arm traces the rays; the lists are built the same way

@pytest.mark.parametrize("name", ["cornell", "ajax_standin_96"])
def test_the_fast_arm_follows_its_own_rays(name):
    scene, r, cam, opt = _open(name)
    try:
        exact = r.id_mattes(cam, opt, 0, PASSES, 8)
        r.set_arithmetic(abi.ARITH_FAST)
        fast = r.id_mattes(cam, opt, 0, PASSES, 8)
    finally:
        r.close()
    _same(fast, _want(name, None, 8, fast=True), name + ", fast arm")
    assert np.array_equal(_bits(fast["total"]), _bits(exact["total"]))
    _same(exact, _want(name), name)


# ---------------------------------------------------------------------------
# 10: the command line

def test_headless_writes_the_lists_of_the_renders_passes(tmp_path, capsys):
    pack = os.path.join(oa.GOLDEN, "cornell.pack")
    path = str(tmp_path/"mattes.npz")
    assert headless.main(["headless", "-spp=4", "-width=%d" % W, "-height=%d" % H, "-mattes=" + path, "-mattes_spp=3", "-mattes_slots=4", pack]) == 0
    assert "wrote " + path in capsys.readouterr().out
    z = np.load(path)
    assert int(z["passes"]) == 3 and sorted(z.files) == ["ids", "passes", "residual", "total", "weights"]
    scene = tinsel_amd.Scene.load_pack(pack)
    cam, opt = _cam_opt(scene)
    opt = _frame(opt, W, H)
    r = tinsel_amd.create_gpu_renderer(scene)
    try:
        r.init(W, H)
        want = r.id_mattes(cam, opt, 0, 3, 4)
        six = r.id_mattes(cam, opt, 0, 2)
    finally:
        r.close()
    _same({k: z[k] for k in KEYS}, want, "headless")
    _same(want, _want("cornell", None, 4), "cornell, 4 slots")
    # the defaults: min(spp, 16) passes, six slots
    assert headless.main(["headless", "-spp=2", "-width=%d" % W, "-height=%d" % H, "-mattes=" + path, pack]) == 0
    z = np.load(path)
    assert int(z["passes"]) == 2 and z["ids"].shape == (6, H, W)
    _same({k: z[k] for k in KEYS}, six, "headless, defaults")
    # a matte of everything that is something is the coverage: one minus the background's
    everything = tinsel_amd.matte(six, np.arange(scene.num_primitives))
    # (the slots and the residual hold the total's terms in another order: 2 passes x 4 x 4 candidates, 2 (n - 1) 2^-24 = 3.7e-6 of the total,
    # and a few roundings of the sums and quotients here)
    seen = six["total"] > 0
    assert seen.sum() > W*H//2 and not tinsel_amd.matte(six, np.arange(-1, scene.num_primitives))[~seen].any()
    rest = np.divide(six["residual"], six["total"], out=np.zeros((H, W), np.float32), where=seen)
    assert np.allclose((everything + tinsel_amd.matte(six, M) + rest)[seen], 1.0, rtol=0, atol=1e-5)

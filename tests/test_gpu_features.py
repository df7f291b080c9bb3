"""Feature buffers (tinsel_hip_render_features / _device, kernel k_features): albedo, normal and depth on the beauty's own samples, bit for bit.

The expected value comes from code that is not under test.  For the path of pixel (i, j) in pass s: the camera record is the one
tests/test_gpu_radiance_query.py::_starts builds from the reference alone (RefOracle.leaf_random, RefOracle.camera_rays, pass_seed); its
first hit is HipRenderer.trace_rays(..., "closest") -- k_query, pinned to the reference's Trace() by tests/test_gpu_ray_query.py --; the
colour is the pack's primitive's.  Per path: albedo = the colour, normal = the record's, depth = (t, t*t, 1) with t*t one float32
multiply, word 3 zero, everything zero at a miss.  The planes are tests/accumulate_reference.add_passes(zeros, feature[passes, H, W, 4],
seeds, filter, clamp = inf): AddSample in numpy float32.  Comparisons are on the uint32 view: every pixel, every word.

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
from tests.test_gpu_radiance_query import _frame, _starts
from tests.test_gpu_ray_query import _cam_opt, _pack, _renderer

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not oa.have_ref(), reason="oracle/_ref not built")]

W, H, PASSES = 50, 37, 3
NAMES = abi.FEATURE_NAMES
BITS = dict(zip(NAMES, (abi.FEATURE_ALBEDO, abi.FEATURE_NORMAL, abi.FEATURE_DEPTH)))
PARITY_SCENES = ["cornell", "glass", "motionblur", "many_spheres", "ajax_standin_96", "cornell_probe", "mesh:beyond_flat:1"] + \
                ["fuzz:%02d" % k for k in range(4)]
G = abi.FILTER_GAUSSIAN
FILTERS = {
    "box_1.0": (abi.FILTER_BOX, 1.0, 1.0, constructor_offset(1.0, 1.0)),
    "gauss_0.75": (G, 0.75, 1.0, constructor_offset(0.75, 1.0)),
    "gauss_1.0_loader": (G, 1.0, 1.0, constructor_offset(0.75, 1.0)),        # the loader keeps Filter(gaussian, 0.75, 1.0)'s offset: the support form
    "gauss_1.5": (G, 1.5, 1.0, constructor_offset(1.5, 1.0)),                # the run-time window
}
FORMS = {"auto": abi.ACCUMULATE_AUTO, "tiled": abi.ACCUMULATE_TILED, "wide": abi.ACCUMULATE_WIDE, "piped": abi.ACCUMULATE_PIPED,
         "full_window": abi.ACCUMULATE_FULL_WINDOW}
# (TINSEL_ACCUMULATE_TILED / _WIDE / _PIPED name kernels for filter widths up to 1: include/tinsel_hip.h)
FILTER_FORMS = [(f, k) for f in FILTERS for k in FORMS if not (FILTERS[f][1] > 1.0 and k in ("tiled", "wide", "piped"))]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what):
    """got: name -> [H, W, 4]; want: the same, of the names asked for"""
    for n, plane in want.items():
        assert got[n].dtype == np.float32 and got[n].shape == plane.shape, (what, n)
        bad = (_bits(got[n]) != _bits(plane)).any(axis=-1)
        assert not bad.any(), "%s, %s: %d of %d pixels differ (first: row %d column %d, %s against %s)" % (
            what, n, int(bad.sum()), bad.size, *np.unravel_index(np.argmax(bad), bad.shape), got[n][np.unravel_index(np.argmax(bad), bad.shape)],
            plane[np.unravel_index(np.argmax(bad), bad.shape)])


def _colours(scene):
    prims = C.cast(scene.desc.primitives, C.POINTER(abi.Primitive))
    return np.array([[prims[k].material.color.x, prims[k].material.color.y, prims[k].material.color.z] for k in range(scene.num_primitives)], np.float32)


def _path_features(r, scene, starts, width, height):
    """name -> [passes, height, width, 4]: the per-path values, from trace_rays on renderer r and the pack's colours"""
    n = len(starts)
    rays = np.zeros((n, 8), np.float32)
    for k, f in enumerate(("ox", "oy", "oz", "time", "dx", "dy", "dz")):
        rays[:, k] = starts[f]
    rays[:, 7] = np.inf
    rec = r.trace_rays(rays, "closest")
    hit = rec["primitive"] >= 0
    out = {name: np.zeros((n, 4), np.float32) for name in NAMES}
    out["albedo"][hit, :3] = _colours(scene)[rec["primitive"][hit]]
    for k, f in enumerate(("nx", "ny", "nz")):
        out["normal"][hit, k] = rec[f][hit]
    t = rec["t"][hit]
    assert t.dtype == np.float32
    out["depth"][hit, 0], out["depth"][hit, 1], out["depth"][hit, 2] = t, t*t, np.float32(1.0)
    return {name: v.reshape(-1, height, width, 4) for name, v in out.items()}, hit.reshape(-1, height, width)


def _planes(paths, seeds, filt, which=NAMES):
    return {n: add_passes(np.zeros(paths[n].shape[1:], np.float32), paths[n], seeds, filt, np.inf) for n in which}


def _filter_of(opt):
    return (opt.filter.type, opt.filter.width, opt.filter.falloff, opt.filter.offset)


@functools.lru_cache(maxsize=None)
def _case(name, pass_begin=0, passes=PASSES):
    """(per-path features, hit mask, seeds, the expected planes under the pack's own filter) of a scene's own camera at 50 x 37: computed
    once, shared, left unchanged"""
    R = oa.RefOracle()
    scene, r = _renderer(name)
    try:
        cam, opt = _cam_opt(scene)
        starts = _starts(R, cam, W, H, pass_begin + passes)[pass_begin*W*H:]
        paths, hit = _path_features(r, scene, starts, W, H)
    finally:
        r.close()
    seeds = tuple(int(R.pass_seed(pass_begin + s)) for s in range(passes))
    want = _planes(paths, seeds, _filter_of(opt))
    for a in list(paths.values()) + list(want.values()) + [hit]:
        a.setflags(write=False)
    return paths, hit, seeds, want


def _open(name, **tuning):
    scene, r = _renderer(name, **tuning)
    cam, opt = _cam_opt(scene)
    opt = _frame(opt, W, H)
    r.init(W, H)
    return scene, r, cam, opt


def _with_filter(opt, filt):
    o = opt.copy()
    o.filter.type, o.filter.width, o.filter.falloff, o.filter.offset = int(filt[0]), float(filt[1]), float(filt[2]), float(filt[3])
    return o


# ---------------------------------------------------------------------------
# 1: parity per scene, the pack's own filter

@pytest.mark.parametrize("name", PARITY_SCENES)
def test_the_planes_are_the_first_hits_accumulated_as_the_beauty_is(name):
    paths, hit, seeds, want = _case(name)
    assert hit.any() and (W*H*PASSES) % 64 != 0
    if name in ("many_spheres", "fuzz:00", "fuzz:01", "fuzz:02"):
        assert not hit.all()                    # rays that leave the scene (a quarter to two thirds of these frames, by the reference's own tables)
    scene, r, cam, opt = _open(name)
    try:
        got = r.features(cam, opt, 0, PASSES)
    finally:
        r.close()
    assert list(got) == list(NAMES)
    _same(got, want, name)
    assert want["albedo"][..., :3].any() and want["depth"][..., 2].any()


# ---------------------------------------------------------------------------
# 2: filters and kernel forms

@pytest.mark.parametrize("filt,form", FILTER_FORMS)
def test_every_filter_and_accumulate_kernel_gives_the_same_planes(filt, form):
    paths, _, seeds, _ = _case("cornell")
    want = _planes(paths, seeds, FILTERS[filt])
    scene, r, cam, opt = _open("cornell")
    try:
        r.set_tuning(accumulate=FORMS[form])
        got = r.features(cam, _with_filter(opt, FILTERS[filt]), 0, PASSES)
    finally:
        r.close()
    _same(got, want, "%s under %s" % (filt, form))


# ---------------------------------------------------------------------------
# 3: the weight plane is the reference accumulator's own

@pytest.mark.parametrize("name", ["cornell", "motionblur"])
def test_the_weight_plane_is_the_reference_accumulators(name):
    R = oa.RefOracle()
    h = R.load_pack(_pack(name))
    try:
        cam, opt = R.camera_options(h)
        accum, _, _ = R.render_seeded(h, cam, _frame(opt, W, H), 0, PASSES, want_accum=True)
    finally:
        R.free(h)
    _, _, _, want = _case(name)
    for n in NAMES:
        assert np.array_equal(_bits(want[n][..., 3]), _bits(accum[..., 3])), n
    scene, r, cam, opt = _open(name)
    try:
        got = r.features(cam, opt, 0, PASSES)
    finally:
        r.close()
    for n in NAMES:
        assert np.array_equal(_bits(got[n][..., 3]), _bits(accum[..., 3])), n


# ---------------------------------------------------------------------------
# 4: pass_begin; what the call leaves alone

def test_pass_begin_names_the_seeds():
    _, _, seeds, want = _case("cornell", 5, 2)
    R = oa.RefOracle()
    assert seeds == (R.pass_seed(5), R.pass_seed(6))
    scene, r, cam, opt = _open("cornell")
    try:
        got = r.features(cam, opt, 5, 2)
        # ... also behind a render that has moved the renderer's own generator past pass 5, and in front of it
        r.render(cam, opt, passes=8)
        again = r.features(cam, opt, 5, 2)
    finally:
        r.close()
    _same(got, want, "passes 5, 6")
    _same(again, want, "passes 5, 6 behind a render of 8")


@pytest.mark.parametrize("lookahead", [0, 1])
def test_a_features_call_between_two_renders_changes_nothing(lookahead):
    _, _, _, want = _case("cornell")
    scene, r, cam, opt = _open("cornell")
    try:
        r.set_lookahead(lookahead)
        r.render(cam, opt, passes=2)
        plain = r.render(cam, opt, passes=2).copy()
        r.init(W, H)
        r.set_pass_index(0)
        r.render(cam, opt, passes=2)
        before = (r.get_pass_index(), r.stats(), r.get_tuning().as_dict())
        got = r.features(cam, opt, 0, PASSES)
        assert (r.get_pass_index(), r.stats(), r.get_tuning().as_dict()) == before and before[0] == 2
        between = r.render(cam, opt, passes=2)
    finally:
        r.close()
    assert between.tobytes() == plain.tobytes()
    _same(got, want, "between two renders")


# ---------------------------------------------------------------------------
# 5: the batch cut

def test_the_batch_cut_shows_nowhere():
    _, _, _, want = _case("cornell")
    scene, r, cam, opt = _open("cornell")
    try:
        r.enable_kernel_timing(True)
        one = r.features(cam, opt, 0, PASSES)
        t1 = r.kernel_times()
        r.set_batch_paths(1024)                 # the smallest the library takes: a pass (1850 slots) per batch
        cut = r.features(cam, opt, 0, PASSES)
        t3 = r.kernel_times()
    finally:
        r.close()
    assert t1["k_features"][0] == 1 and t3["k_features"][0] == PASSES >= 2
    _same(one, want, "one batch")
    _same(cut, one, "three batches")


# ---------------------------------------------------------------------------
# 6: the mask

def test_the_mask_selects_planes_in_bit_order():
    scene, r, cam, opt = _open("glass")
    try:
        full = r.features(cam, opt, 0, PASSES)
        for n in NAMES:
            got = r.features(cam, opt, 0, PASSES, which=(n,))
            assert list(got) == [n]
            _same(got, {n: full[n]}, "only " + n)
        for pair in (("albedo", "normal"), ("depth", "albedo"), ("depth", "normal")):
            raw = np.full((2, H, W, 4), 7.0, np.float32)
            got = r.features(cam, opt, 0, PASSES, which=pair, out=raw)
            order = [n for n in NAMES if n in pair]
            assert list(got) == order
            for k, n in enumerate(order):                  # ascending bit order in the array itself, whatever order the caller names them in
                assert np.array_equal(_bits(raw[k]), _bits(full[n])), (pair, n)
            mask = BITS[pair[0]] | BITS[pair[1]]
            assert tinsel_amd.feature_mask(pair) == (mask, order) and tinsel_amd.feature_mask(mask) == (mask, order)
    finally:
        r.close()
    _same(full, _case("glass")[3], "glass")


# ---------------------------------------------------------------------------
# 7: shards

@pytest.mark.parametrize("world", [2, 3])
def test_the_shards_planes_sum_to_the_frames(world):
    box = FILTERS["box_1.0"]
    scene, r, cam, opt = _open("cornell")
    opt = _with_filter(opt, box)
    try:
        whole = r.features(cam, opt, 0, PASSES)
        parts = []
        for rank in range(world):
            r.set_shard(rank, world, 16)
            parts.append(r.features(cam, opt, 0, PASSES))
    finally:
        r.close()
    paths, _, seeds, _ = _case("cornell")
    _same(whole, _planes(paths, seeds, box), "the whole frame, box filter")
    total = {n: sum(p[n].astype(np.float64) for p in parts) for n in NAMES}
    for n in NAMES:
        k = whole[n][..., 3].astype(np.float64)
        # the weights (and the depth plane's hit count) are small integers: exact whatever the order
        assert np.array_equal(total[n][..., 3], k), n
        assert any(p[n][..., 3].any() for p in parts) and not all((p[n][..., 3] == whole[n][..., 3]).all() for p in parts)
    assert np.array_equal(total["depth"][..., 2], whole["depth"][..., 2].astype(np.float64))
    # terms of magnitude at most 1, at most k of them, each add rounding by at most 2^-24 * k, two summation orders
    for n in ("albedo", "normal"):
        k = whole[n][..., 3].astype(np.float64)
        err = np.abs(total[n][..., :3] - whole[n][..., :3].astype(np.float64)).max(axis=-1)
        print("%s, world %d: largest error %.3g, bound at that pixel %.3g" % (n, world, err.max(), (k*k*2.0**-23).ravel()[np.argmax(err)]))
        assert (err <= k*k*2.0**-23).all(), n


# ---------------------------------------------------------------------------
# 8: the scene in force

def test_a_moved_primitive_is_refused_until_the_rebuild_and_seen_after_it():
    R = oa.RefOracle()
    scene, r, cam, opt = _open("cornell")
    L, hnd = r._L, r._h
    try:
        still = r.features(cam, opt, 0, PASSES)
        last = scene.num_primitives - 1
        t = abi.Transform.from_buffer_copy(bytes(C.cast(scene.desc.primitives, C.POINTER(abi.Primitive))[last].start_transform))
        t.p.x += 0.25
        r.set_primitive_transform(last, t, t)
        out = np.full((3, H, W, 4), 5.0, np.float32)
        assert L.tinsel_hip_render_features(hnd, C.byref(cam), C.byref(opt), 0, PASSES, 7, out.ctypes.data_as(C.c_void_p)) == -1
        msg = L.tinsel_hip_last_error()
        assert msg.startswith(b"render_features:") and b"call tinsel_hip_rebuild_scene first" in msg and (out == 5.0).all()
        r.rebuild_scene()
        got = r.features(cam, opt, 0, PASSES)
        paths, _ = _path_features(r, scene, _starts(R, cam, W, H, PASSES), W, H)        # trace_rays on the moved scene
    finally:
        r.close()
    seeds = [R.pass_seed(s) for s in range(PASSES)]
    _same(got, _planes(paths, seeds, _filter_of(opt)), "the moved scene")
    assert any((_bits(got[n]) != _bits(still[n])).any() for n in NAMES)


# ---------------------------------------------------------------------------
# 9: the device entry

def test_the_device_entry_on_a_side_stream():
    torch = pytest.importorskip("torch")
    scene, r, cam, opt = _open("ajax_standin_96")
    try:
        host = r.features(cam, opt, 0, PASSES)
        dev = torch.full((4, H, W, 4), 9.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            got = r.features(cam, opt, 0, PASSES, out=dev[:3])
        beauty = r.render(cam, opt, passes=1)         # enqueued right behind it on the renderer's own stream: no synchronise in between
        side.synchronize()
        assert all(got[n].is_cuda for n in NAMES)
        _same({n: got[n].cpu().numpy() for n in NAMES}, host, "device entry")
        assert (dev[3].cpu().numpy() == 9.0).all() and np.isfinite(beauty).all()
        # two planes, on another stream right behind the first call: the later call waits for the earlier one's buffers
        other = torch.cuda.Stream()
        dev2 = torch.full((2, H, W, 4), 9.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            first = r.features(cam, opt, 0, PASSES, out=dev[:3])
        with torch.cuda.stream(other):
            second = r.features(cam, opt, 0, PASSES, which=("normal", "depth"), out=dev2)
        torch.cuda.synchronize()
        _same({n: second[n].cpu().numpy() for n in ("normal", "depth")}, {n: host[n] for n in ("normal", "depth")}, "second stream")
        _same({n: first[n].cpu().numpy() for n in NAMES}, host, "first stream")
    finally:
        r.close()
    _same(host, _case("ajax_standin_96")[3], "ajax_standin_96")


# ---------------------------------------------------------------------------
# 10: refusals

def test_refusals_write_nothing():
    torch = pytest.importorskip("torch")
    scene, r, cam, opt = _open("cornell")
    fresh_scene, fresh = _renderer("cornell")           # never init-ed
    L, hnd = r._L, r._h
    out = np.full((3, H, W, 4), 5.0, np.float32)
    op = out.ctypes.data_as(C.c_void_p)
    dev = torch.full((3*H*W*4 + 8,), 5.0, dtype=torch.float32, device="cuda")
    normals, wrong = opt.copy(), opt.copy()
    normals.mode = abi.MODE_NORMALS
    wrong.width = W + 1
    cp, opp = C.byref(cam), C.byref(opt)
    try:
        cases = [
            ("null", (None, cp, opp, 0, PASSES, 7, op)),
            ("null", (hnd, None, opp, 0, PASSES, 7, op)),
            ("null", (hnd, cp, None, 0, PASSES, 7, op)),
            ("null", (hnd, cp, opp, 0, PASSES, 7, None)),
            ("passes", (hnd, cp, opp, 0, 0, 7, op)),
            ("passes", (hnd, cp, opp, 0, -3, 7, op)),
            ("features", (hnd, cp, opp, 0, PASSES, 0, op)),
            ("features", (hnd, cp, opp, 0, PASSES, 8, op)),
            ("mode", (hnd, cp, C.byref(normals), 0, PASSES, 7, op)),
            ("width/height", (hnd, cp, C.byref(wrong), 0, PASSES, 7, op)),
            ("width/height", (fresh._h, cp, opp, 0, PASSES, 7, op)),
        ]
        for cause, args in cases:
            assert L.tinsel_hip_init(None, 0, 0) == -1 and L.tinsel_hip_last_error().startswith(b"init:")      # another entry's text in between
            assert L.tinsel_hip_render_features(*args) == -1, (cause, args)
            msg = L.tinsel_hip_last_error()
            assert msg.startswith(b"render_features:") and cause.encode() in msg, msg
            assert (out == 5.0).all()
            dargs = args[:6] + (dev.data_ptr() if args[6] is not None else None, None)
            assert L.tinsel_hip_render_features_device(*dargs) == -1, (cause, dargs)
            msg = L.tinsel_hip_last_error()
            assert msg.startswith(b"render_features_device:") and cause.encode() in msg, msg
        # the device entry's own: an output that is not 16-byte aligned
        assert L.tinsel_hip_render_features_device(hnd, cp, opp, 0, PASSES, 7, dev.data_ptr() + 4, None) == -1
        msg = L.tinsel_hip_last_error()
        assert msg.startswith(b"render_features_device:") and b"16-byte aligned" in msg
        torch.cuda.synchronize()
        assert (dev.cpu().numpy() == 5.0).all()
        # (a moved primitive without the rebuild: test_a_moved_primitive_is_refused_until_the_rebuild_and_seen_after_it)
        assert L.tinsel_hip_render_features(hnd, cp, opp, 0, PASSES, 7, op) == 0 and not (out == 5.0).all()
    finally:
        r.close()
        fresh.close()


# ---------------------------------------------------------------------------
# 11: kernel times

@pytest.mark.parametrize("which", [NAMES, ("normal",), ("albedo", "depth")])
def test_kernel_times_list_the_calls_kernels(which):
    scene, r, cam, opt = _open("cornell")
    try:
        r.enable_kernel_timing(True)
        r.render(cam, opt, passes=1)
        r.features(cam, opt, 0, PASSES, which=which)
        one = r.kernel_times()
        r.set_batch_paths(1024)
        r.features(cam, opt, 0, PASSES, which=which)
        three = r.kernel_times()
    finally:
        r.close()
    # the call's own record: nothing of the render before it
    assert sorted(one) == sorted(three) == ["k_accumulate", "k_features"]
    assert one["k_features"][0] == 1 and one["k_accumulate"][0] == len(which)
    assert three["k_features"][0] == PASSES and three["k_accumulate"][0] == len(which)*PASSES
    assert one["k_features"][1] > 0 and one["k_accumulate"][1] > 0


# ---------------------------------------------------------------------------
# 12: the fast arithmetic arm

@pytest.mark.parametrize("name", ["cornell", "ajax_standin_96"])
def test_the_fast_arm_answers_with_the_same_shapes(name):
    """shapes, finiteness and weights only; the planes' values against the exact arm's, pixel by pixel off the edges:
    tests/test_gpu_fast_accuracy.py::test_feature_planes_follow_the_exact_arm_off_the_edges"""
    scene, r, cam, opt = _open(name)
    try:
        exact = r.features(cam, opt, 0, PASSES)
        r.set_arithmetic(abi.ARITH_FAST)
        fast = r.features(cam, opt, 0, PASSES)
    finally:
        r.close()
    assert list(fast) == list(exact)
    for n in NAMES:
        assert fast[n].shape == exact[n].shape and fast[n].dtype == np.float32
        assert np.isfinite(fast[n]).all()
        assert (fast[n][..., 3][exact[n][..., 3] > 0] > 0).all()
    assert fast["depth"][..., 2].any()


# ---------------------------------------------------------------------------
# 13: the command line

def test_headless_writes_the_planes_of_the_renders_passes(tmp_path, capsys):
    pack = os.path.join(oa.GOLDEN, "cornell.pack")
    path = str(tmp_path/"features.npz")
    assert headless.main(["headless", "-spp=4", "-width=%d" % W, "-height=%d" % H, "-features=" + path, "-features_spp=3", pack]) == 0
    assert "wrote " + path in capsys.readouterr().out
    z = np.load(path)
    assert int(z["passes"]) == 3
    scene = tinsel_amd.Scene.load_pack(pack)
    cam, opt = _cam_opt(scene)
    opt = _frame(opt, W, H)
    r = tinsel_amd.create_gpu_renderer(scene)
    try:
        r.init(W, H)
        want = r.features(cam, opt, 0, 3)
    finally:
        r.close()
    _same({n: z[n + "_plane"] for n in NAMES}, want, "headless")
    images = tinsel_amd.feature_images(want)
    assert sorted(images) == ["albedo", "coverage", "depth", "depth_variance", "normal"]
    for k, v in images.items():
        assert np.array_equal(z[k], v), k
    _same(want, _case("cornell")[3], "cornell")
    # the default: min(spp, 16) passes
    assert headless.main(["headless", "-spp=2", "-width=%d" % W, "-height=%d" % H, "-features=" + path, pack]) == 0
    assert int(np.load(path)["passes"]) == 2

"""Radiance queries (tinsel_hip_trace_radiance / _device, kernel k_generate_rays) against the reference's PathTrace, bit for bit.

Expected values come from the reference alone.  For the path of pixel (i, j) in pass s of a W x H frame: seed = i + j*W + pass_seed(s);
the three draws x, y, t are outputs 0..2 of leaf_random(seed, 3) run through Randf(0, 1)'s float32 expression, (1 - r)*0 + r*1; the raster
position is (x + i, y + j) in float32; the ray is RefOracle.camera_rays of that position; the time the reference's Lerp of the shutter,
a + (b - a)*t in float32; the generator words rng_state(seed, 3).  The expected radiance of that record is
render_seeded(..., want_radiance=True)[1][s, j, i], and the comparison is on the uint32 view of the three floats: every path, every bit.

The frame is 50 x 37 with 3 passes: n = 5550 paths, no multiple of 64, several regions.  max_depth is the pack's own."""
import ctypes as C
import functools

import numpy as np
import pytest

import tinsel_amd
from tinsel_amd import abi
from tests import oracle_api as oa
from tests.test_gpu_ray_query import _cam_opt, _pack, _renderer

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not oa.have_ref(), reason="oracle/_ref not built")]

W, H, PASSES = 50, 37, 3
N = W*H*PASSES
PARITY_SCENES = ["cornell", "glass", "veach", "features", "motionblur", "many_spheres", "cornell_probe", "ajax_standin_96"] + \
                ["fuzz:%02d" % k for k in range(8)] + ["mesh:instances:1", "mesh:beyond_flat:1"]
PIPELINES = {"auto": abi.PIPELINE_AUTO, "wavefront": abi.PIPELINE_WAVEFRONT, "split": abi.PIPELINE_WAVEFRONT_SPLIT,
             "paired": abi.PIPELINE_WAVEFRONT_PAIRED, "megakernel": abi.PIPELINE_MEGAKERNEL}


@pytest.fixture(scope="module")
def ref():
    return oa.RefOracle()


@functools.lru_cache(maxsize=None)
def _draws(width, height, passes):
    """What does not depend on the scene or the camera, per path in slot order (pass, row, column): pixel, the three camera draws, the
    generator words PathTrace is entered with"""
    R = oa.RefOracle()
    jj, ii = np.mgrid[0:height, 0:width]
    i, j = ii.ravel().astype(np.uint32), jj.ravel().astype(np.uint32)
    pix, draws, words = [], [], []
    for s in range(passes):
        seed = i + j*np.uint32(width) + np.uint32(R.pass_seed(s))                  # (uint32: wraps as the reference's int does)
        r = np.stack([R.leaf_random(int(k), 3)[1] for k in seed])                   # Randf() outputs 0..2
        assert r.dtype == np.float32
        draws.append((np.float32(1.0) - r)*np.float32(0.0) + r*np.float32(1.0))     # Randf(0, 1)
        pix.append(np.stack([i, j], axis=1))
        words.append(np.stack(tinsel_amd.rng_state(seed, 3), axis=1))
    return np.concatenate(pix), np.concatenate(draws), np.concatenate(words)


def _starts(R, cam, width=W, height=H, passes=PASSES):
    """the records of the camera's own paths, in slot order"""
    pix, draws, words = _draws(width, height, passes)
    assert draws.dtype == np.float32
    raster = (draws[:, 0:2] + pix.astype(np.float32)).astype(np.float32)
    od = R.camera_rays(cam, width, height, raster)
    a, b = np.float32(cam.shutter_start), np.float32(cam.shutter_end)
    starts = np.zeros(len(pix), abi.PATH_START_DTYPE)
    starts["ox"], starts["oy"], starts["oz"] = od[:, 0], od[:, 1], od[:, 2]
    starts["dx"], starts["dy"], starts["dz"] = od[:, 3], od[:, 4], od[:, 5]
    starts["time"] = a + (b - a)*draws[:, 2]
    starts["rng1"], starts["rng2"] = words[:, 0], words[:, 1]
    return starts


def _frame(opt, width=W, height=H):
    o = opt.copy()
    o.width, o.height = width, height
    return o


def _expected(O, h, cam, opt, passes=PASSES):
    """the reference's PathTrace value of every path of the frame, in slot order, padded to the output's four words"""
    _, rad, _ = O.render_seeded(h, cam, opt, 0, passes, want_accum=False, want_radiance=True)
    return np.ascontiguousarray(rad.reshape(-1, 3))


def _same(got, want, what):
    assert got.dtype == np.float32 and got.shape == (len(want), 4), what
    a, b = np.ascontiguousarray(got[:, :3]).view(np.uint32), want.view(np.uint32)
    bad = (a != b).any(axis=1)
    assert not bad.any(), "%s: %d of %d paths differ from the reference (first: record %d, %s against %s)" % (
        what, int(bad.sum()), len(want), int(np.argmax(bad)), got[np.argmax(bad), :3], want[np.argmax(bad)])


@functools.lru_cache(maxsize=None)
def _case(name):
    """(starts, expected, max_depth) of a scene's own camera: computed once, shared, left unchanged"""
    R = oa.RefOracle()
    h = R.load_pack(_pack(name))
    cam, opt = R.camera_options(h)
    opt = _frame(opt)
    starts, want = _starts(R, cam), _expected(R, h, cam, opt)
    R.free(h)
    starts.setflags(write=False)
    want.setflags(write=False)
    return starts, want, opt.max_depth


# ---------------------------------------------------------------------------
# 1: parity with the scene's own camera

@pytest.mark.parametrize("name", PARITY_SCENES)
def test_the_camera_paths_as_a_query_are_the_reference_radiance(name):
    starts, want, depth = _case(name)
    assert want.any() and N % 64 != 0
    scene, r = _renderer(name)
    try:
        s0 = r.stats()
        got = r.radiance(starts, depth)                 # (a renderer that was never init-ed answers)
        s1 = r.stats()
    finally:
        r.close()
    _same(got, want, name)
    # a query is path tracing: its paths and rays are counted
    assert s1["samples"] - s0["samples"] == N and s1["rays"] - s0["rays"] >= N


# ---------------------------------------------------------------------------
# 2: rays a render never makes

def _random_cameras(R, h, count, seed):
    rng = np.random.default_rng(seed)
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for p in range(R.num_primitives(h)):
        if R.primitive(h, p).type != abi.GEOM_PLANE:
            a, b = R.primitive_bounds(h, p)
            lo, hi = np.minimum(lo, a), np.maximum(hi, b)
    size = hi - lo
    lo, hi = lo - 0.5*size, hi + 0.5*size
    base, _ = R.camera_options(h)
    cams = []
    for _ in range(count):
        cam = abi.Camera.from_buffer_copy(bytes(base))
        pos = lo + rng.random(3)*(hi - lo)
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        cam.position.x, cam.position.y, cam.position.z = (float(np.float32(v)) for v in pos)
        cam.rotation.x, cam.rotation.y, cam.rotation.z, cam.rotation.w = (float(np.float32(v)) for v in q)
        cam.fov = float(np.float32(np.radians(rng.uniform(20.0, 120.0))))
        cams.append(cam)
    return cams


@pytest.mark.parametrize("name", ["cornell", "glass", "many_spheres"])
def test_paths_from_cameras_the_scene_does_not_have(ref, name):
    h = ref.load_pack(_pack(name))
    _, opt = ref.camera_options(h)
    opt = _frame(opt)
    scene, r = _renderer(name)
    try:
        for k, cam in enumerate(_random_cameras(ref, h, 4, 20261018 + PARITY_SCENES.index(name))):
            starts, want = _starts(ref, cam), _expected(ref, h, cam, opt)
            assert not np.array_equal(starts["ox"], _case(name)[0]["ox"])
            _same(r.radiance(starts, opt.max_depth), want, "%s camera %d" % (name, k))
    finally:
        r.close()
        ref.free(h)


# ---------------------------------------------------------------------------
# 3: order and cut do not matter

def test_order_and_cut_do_not_matter():
    starts, want, depth = _case("veach")
    scene, r = _renderer("veach")
    try:
        whole = r.radiance(starts, depth)
        _same(whole, want, "veach")
        perm = np.random.default_rng(5).permutation(N)
        assert r.radiance(starts[perm], depth).tobytes() == whole[perm].tobytes()
        # the same records as (n, 12) words
        words = np.ascontiguousarray(starts).view(np.uint32).reshape(N, 12)
        assert r.radiance(words, depth).tobytes() == whole.tobytes()
        for n in (0, 1, 63, 65):
            assert r.radiance(starts[:n], depth).tobytes() == whole[:n].tobytes(), n
        # three batches, the last one ragged, against the one-batch query of the same records
        long = np.concatenate([starts, starts[:4000]])
        one = r.radiance(long, depth)
        assert one.tobytes() == np.concatenate([whole, whole[:4000]]).tobytes()
        r.set_batch_paths(4096)
        assert 2*4096 < len(long) < 3*4096 and len(long) % 4096 != 0
        assert r.radiance(long, depth).tobytes() == one.tobytes()
        assert r.radiance(starts, depth).tobytes() == whole.tobytes()           # two batches
    finally:
        r.close()


def test_the_host_entry_across_its_chunk():
    """The host entry stages 2^20 records at a time (kRadianceChunk, tn_host_radiance.h): the reference records of the frame, tiled past the cut,
    give the reference bytes tiled the same way -- a path's result is a function of its record alone."""
    starts, want, depth = _case("cornell")
    chunk = 2**20
    n = chunk + 17
    assert chunk < n < 2*chunk and n % N != 0
    pick = np.arange(n) % N
    scene, r = _renderer("cornell")
    try:
        got = r.radiance(starts[pick], depth)
    finally:
        r.close()
    assert got.dtype == np.float32 and got.shape == (n, 4)
    assert np.ascontiguousarray(got[:, :3]).tobytes() == want[pick].tobytes()


def test_guard_words_reserved_words_and_refusals():
    starts, want, depth = _case("cornell")
    scene, r = _renderer("cornell")
    L, hnd = r._L, r._h
    try:
        whole = r.radiance(starts[:200], depth)
        # reserved words are ignored on input
        noisy = starts[:200].copy()
        noisy["reserved0"], noisy["reserved1"], noisy["reserved2"] = np.nan, 0xdeadbeef, 7
        assert r.radiance(noisy, depth).tobytes() == whole.tobytes()
        # nothing is written behind the n-th record, nor into the records
        inp = np.ascontiguousarray(starts[:72]).copy()
        out = np.full((72, 4), 3.0, np.float32)
        assert L.tinsel_hip_trace_radiance(hnd, 65, inp.ctypes.data_as(C.c_void_p), depth, out.ctypes.data_as(C.c_void_p)) == 0
        assert out[:65].tobytes() == whole[:65].tobytes() and (out[65:] == 3.0).all() and inp.tobytes() == starts[:72].tobytes()
        sp, op = inp.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
        assert L.tinsel_hip_trace_radiance(hnd, 0, None, depth, None) == 0
        cases = [lambda: L.tinsel_hip_trace_radiance(hnd, 8, None, depth, op), lambda: L.tinsel_hip_trace_radiance(hnd, 8, sp, depth, None),
                 lambda: L.tinsel_hip_trace_radiance(hnd, -1, sp, depth, op), lambda: L.tinsel_hip_trace_radiance(hnd, 8, sp, 0, op)]
        for k, case in enumerate(cases):
            out[:] = 5.0
            assert case() == -1 and L.tinsel_hip_last_error().startswith(b"trace_radiance:"), k
            assert (out == 5.0).all()
        # between a move and the rebuild the scene is not in force: refused in query_ready's words
        last = scene.desc.num_primitives - 1
        t = abi.Transform.from_buffer_copy(bytes(C.cast(scene.desc.primitives, C.POINTER(abi.Primitive))[last].start_transform))
        t.p.x += 0.25
        r.set_primitive_transform(last, t, t)
        assert L.tinsel_hip_trace_radiance(hnd, 8, sp, depth, op) == -1
        msg = L.tinsel_hip_last_error()
        assert msg.startswith(b"trace_radiance:") and b"call tinsel_hip_rebuild_scene first" in msg and (out == 5.0).all()
        r.rebuild_scene()
        assert L.tinsel_hip_trace_radiance(hnd, 8, sp, depth, op) == 0
    finally:
        r.close()


# ---------------------------------------------------------------------------
# 4: every pipeline setting

@pytest.mark.parametrize("setting", list(PIPELINES))
@pytest.mark.parametrize("name", ["cornell", "ajax_standin_96"])
def test_every_pipeline_setting_gives_the_reference_bytes(name, setting):
    starts, want, depth = _case(name)
    scene, r = _renderer(name)
    try:
        r.set_pipeline(PIPELINES[setting])
        r.enable_kernel_timing(True)
        got = r.radiance(starts, depth)
        times = r.kernel_times()
    finally:
        r.close()
    _same(got, want, "%s under %s" % (name, setting))
    assert times["k_generate_rays"][0] == 1 and times["k_generate_rays"][1] > 0, times
    assert "k_bounce" not in times and "k_mega" not in times and "k_generate" not in times, times
    if setting == "paired":         # (both scenes are flat-scan scenes: the paired pipeline takes them)
        assert "k_step" in times and "k_shade" not in times, times
    if setting in ("wavefront", "split", "megakernel"):
        assert "k_shade" in times and "k_step" not in times, times


# ---------------------------------------------------------------------------
# 5: a query disturbs nothing

@pytest.mark.parametrize("lookahead", [0, 1], ids=["plain", "lookahead"])
def test_a_query_between_two_renders_disturbs_nothing(lookahead):
    starts, want, depth = _case("cornell")
    scene, r = _renderer("cornell")
    cam, opt = _cam_opt(scene)
    opt = _frame(opt, 64, 48)
    try:
        r.init(64, 48)
        whole = r.render(cam, opt, passes=2).copy()
        r.init(64, 48)
        r.set_pass_index(0)
        r.set_lookahead(lookahead)
        first = r.render(cam, opt, passes=1).copy()
        before = (r.get_pass_index(), r.get_tuning().as_dict())
        got = r.radiance(starts, depth)
        assert (r.get_pass_index(), r.get_tuning().as_dict()) == before and before[0] == 1
        if not lookahead:
            assert r.read_accum().tobytes() == first.tobytes()
        out = r.render(cam, opt, passes=1)
        assert r.get_pass_index() == 2
    finally:
        r.close()
    _same(got, want, "cornell between renders")
    assert not np.array_equal(first, whole) and out.tobytes() == whole.tobytes()


# ---------------------------------------------------------------------------
# 6: the device entry

def test_the_device_entry_on_a_side_stream_and_a_render_right_behind_it():
    import torch
    name = "ajax_standin_96"            # (a render runs the pipeline a query runs: the path buffers are shared, nothing is allocated in between)
    starts, want, depth = _case(name)
    scene, r = _renderer(name)
    cam, opt = _cam_opt(scene)
    opt = _frame(opt)
    try:
        many = np.concatenate([starts]*8)
        host = r.radiance(many, depth)          # (the largest batch first: the buffers are allocated here)
        _same(host[:N], want, name)
        r.init(W, H)
        acc = r.render(cam, opt, passes=1).copy()
        r.init(W, H)
        r.set_pass_index(0)
        words = np.ascontiguousarray(many).view(np.float32).reshape(len(many), 12)
        dev = torch.from_numpy(np.concatenate([words, np.full((4, 12), 7.0, np.float32)])).cuda()
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            out = r.radiance(dev[:len(many)], depth)
        again = r.render(cam, opt, passes=1)    # enqueued right behind the query: no synchronise in between
        side.synchronize()
        assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (len(many), 4)
        assert out.cpu().numpy().tobytes() == host.tobytes()
        assert again.tobytes() == acc.tobytes()
        assert (dev[len(many):].cpu().numpy() == 7.0).all() and dev[:len(many)].cpu().numpy().tobytes() == words.tobytes()
        # and the other way round: a query enqueued right behind a render on another stream
        r.init(W, H)
        r.set_pass_index(0)
        other = torch.cuda.Stream()
        r.render_async(cam, opt, passes=1, stream=other.cuda_stream)
        with torch.cuda.stream(side):
            out2 = r.radiance(dev[:len(many)], depth)
        torch.cuda.synchronize()
        assert out2.cpu().numpy().tobytes() == host.tobytes() and r.read_accum().tobytes() == acc.tobytes()
        # guard words behind the device output; misaligned and overlapping arrays are refused
        guard = torch.full((N + 4, 4), 3.0, dtype=torch.float32, device="cuda")
        L, hnd = r._L, r._h
        assert L.tinsel_hip_trace_radiance_device(hnd, N, dev.data_ptr(), depth, guard.data_ptr(), None) == 0
        torch.cuda.synchronize()
        g = guard.cpu().numpy()
        assert g[:N].tobytes() == host[:N].tobytes() and (g[N:] == 3.0).all()
        for bad in (lambda: L.tinsel_hip_trace_radiance_device(hnd, N, dev.data_ptr() + 4, depth, guard.data_ptr(), None),
                    lambda: L.tinsel_hip_trace_radiance_device(hnd, N, dev.data_ptr(), depth, guard.data_ptr() + 8, None),
                    lambda: L.tinsel_hip_trace_radiance_device(hnd, N, dev.data_ptr(), depth, dev.data_ptr() + 1024, None),
                    lambda: L.tinsel_hip_trace_radiance_device(hnd, N, None, depth, guard.data_ptr(), None),
                    lambda: L.tinsel_hip_trace_radiance_device(hnd, N, dev.data_ptr(), 0, guard.data_ptr(), None)):
            assert bad() == -1 and L.tinsel_hip_last_error().startswith(b"trace_radiance_device:")
        torch.cuda.synchronize()
        assert guard.cpu().numpy()[:N].tobytes() == host[:N].tobytes()
        assert len(r.radiance(dev[:0], depth)) == 0
    finally:
        r.close()


# ---------------------------------------------------------------------------
# 7: roulette and arithmetic

def test_the_query_follows_the_roulette_setting(ref):
    from tests.test_gpu_roulette import _port
    name = "glass"
    P = _port()
    h = P.load_pack(_pack(name))
    cam, opt = P.camera_options(h)
    opt = _frame(opt)
    try:
        P.lib.port_set_russian_roulette(3)
        want = _expected(P, h, cam, opt)
    finally:
        P.lib.port_set_russian_roulette(0)
        P.free(h)
    starts, plain, depth = _case(name)
    assert not np.array_equal(want, plain)              # the rule does something
    scene, r = _renderer(name)
    try:
        r.set_russian_roulette(3)
        got = r.radiance(starts, depth)
        r.set_russian_roulette(0)
        off = r.radiance(starts, depth)
    finally:
        r.close()
    _same(got, want, "glass, roulette from bounce 3")
    _same(off, plain, "glass, roulette off again")


def test_the_fast_arithmetic_arm_answers():
    """that the entry answers under the tolerance arm at all; WHAT it answers -- per path, by depth, under every pipeline -- is held in
    tests/test_gpu_fast_accuracy.py (test_paths_stay_on_track_and_the_rest_is_unbiased, test_paths_under_every_pipeline)"""
    starts, want, depth = _case("cornell")
    scene, r = _renderer("cornell")
    try:
        r.set_arithmetic(abi.ARITH_FAST)
        got = r.radiance(starts, depth)
    finally:
        r.close()
    assert got.shape == (N, 4) and np.isfinite(got).all() and got[:, :3].any()

"""SH gather queries (tinsel_hip_gather_sh / _device; kernel k_gather_sh_reduce): a gather query's paths projected onto the real spherical
harmonics of bands 0 .. order, reduced on the device.

As test_gpu_gather.py: the points are the first-hit points of a pack's own camera at 16 x 12, max_depth is 4, and what the query returns is
held to what the library already answers for the SAME paths one by one -- gather_sh(..., return_starts=True) gives the generated records,
radiance() of those records (held to the reference bit for bit by test_gpu_radiance_query.py) gives L_s, sh_basis of the records' float32
directions gives Y_i(d_s), and the float32 products summed sequentially in s (np.add.accumulate) and divided by float32(S) must be the
query's coefficients, bit for bit.  The sample counts 1, 5, 64, 67 and 130 are a partial chunk of the kernel's 64-sample chunks, an exact
one, one and a tail, and several."""
import ctypes as C
import os

import numpy as np
import pytest

import tinsel_amd
from tinsel_amd import abi
from tests import oracle_api as oa
from tests.test_gpu_gather import _surface
from tests.test_gpu_ray_query import _cam_opt, _renderer

pytestmark = pytest.mark.gpu

W, H, DEPTH = 16, 12, 4
SAMPLES = (1, 5, 64, 67, 130)
ORDERS = (0, 1, 2)
MODES = ("cosine", "sphere")
Y0 = np.float32(0.28209479)


def _contract(r, starts, n, samples, order):
    """the stated sum: float32 products L_s * Y_i(d_s), added in ascending s in float32, divided by float32(samples): [n, C, 3]"""
    rad = r.radiance(starts, DEPTH)
    d = np.stack([starts["dx"], starts["dy"], starts["dz"]], axis=-1)
    assert d.dtype == np.float32
    Y = tinsel_amd.sh_basis(d, order)
    coeffs = Y.shape[1]
    prod = (rad[:, None, :3]*Y[:, :, None]).reshape(n, samples, coeffs, 3)
    assert prod.dtype == np.float32
    total = np.add.accumulate(prod, axis=1, dtype=np.float32)[:, -1]
    assert total.dtype == np.float32
    return total/np.float32(samples)


def _hold(r, pts, samples, order, mode, what):
    n, coeffs = len(pts), (order + 1)**2
    coef, starts = r.gather_sh(pts, samples, DEPTH, order, mode, return_starts=True)
    assert coef.dtype == np.float32 and coef.shape == (n, coeffs, 4) and starts.shape == (n*samples,)
    want = _contract(r, starts, n, samples, order)
    assert np.isfinite(want).all() and want.any(), what
    differ = (coef[..., :3] != want).any(axis=(1, 2))
    print("%s: %d of %d points differ, largest difference %g" % (what, int(differ.sum()), n, float(np.abs(coef[..., :3] - want).max())))
    assert np.array_equal(coef[..., :3], want), "%s: %d of %d points differ from the sequential sum (largest difference %g)" % (
        what, int(differ.sum()), n, float(np.abs(coef[..., :3] - want).max()))
    assert (coef[..., 3].view(np.uint32) == 0).all(), what
    return coef, starts


# ---------------------------------------------------------------------------
# 1: the contract, bit for bit

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["cornell", "ajax_standin_96", "motionblur", "cornell_probe"])
def test_the_coefficients_are_the_sequential_sum_of_radiance_times_basis(name, mode):
    pos, nrm = _surface(name)
    scene, r = _renderer(name)
    try:
        if name == "ajax_standin_96":
            assert r.walked_prims > 0                   # (the paired pipeline: k_walk + k_step behind k_generate_gather)
        cam, _ = _cam_opt(scene)
        times = 1.0
        if name == "motionblur":
            assert cam.shutter_end > cam.shutter_start
            times = np.linspace(cam.shutter_start, cam.shutter_end, len(pos)).astype(np.float32)
        for samples in SAMPLES:
            pts = tinsel_amd.gather_points(pos, nrm, samples, time=times, base_seed=1000*samples)
            for order in ORDERS:
                _hold(r, pts, samples, order, mode, "%s %s order %d S=%d" % (name, mode, order, samples))
    finally:
        r.close()


# ---------------------------------------------------------------------------
# 2: the starts are the gather query's

@pytest.mark.parametrize("mode", MODES)
def test_the_starts_are_the_gather_querys(mode):
    pos, nrm = _surface("cornell")
    samples = 67
    seeds = (np.arange(len(pos), dtype=np.uint64)*np.uint64(977) + np.uint64(31)).astype(np.uint32)
    seeds[:3] = [2**32 - 1, 2**32 - 3, 0]                       # seed + s wraps in 32 bits
    pts = tinsel_amd.gather_points(pos, nrm, samples, time=np.linspace(0.0, 1.0, len(pos)).astype(np.float32), seeds=seeds)
    scene, r = _renderer("cornell")
    try:
        _, plain = r.gather(pts, samples, DEPTH, mode, return_starts=True)
        _, sh = r.gather_sh(pts, samples, DEPTH, 2, mode, return_starts=True)
    finally:
        r.close()
    assert plain["rng1"].any() and sh.tobytes() == plain.tobytes()


# ---------------------------------------------------------------------------
# 3: band 0 against the existing mean

@pytest.mark.parametrize("arith", ["exact", "fast"])
def test_band_zero_is_the_gathers_mean_times_y0(arith):
    """coef[:, 0, c] and Y0 * mean_c are two sequential fp32 sums of S non-negative terms (S - 1 roundings each, every partial sum no larger
    than the total), the one of products rounded once each, then a divide each, and the product with Y0: (2S + 4) * 2^-24 relative.  The fast
    arm carries no bit contract; this is its check."""
    pos, nrm = _surface("cornell")
    scene, r = _renderer("cornell")
    try:
        if arith == "fast":
            r.set_arithmetic(abi.ARITH_FAST)
        for mode in MODES:
            for samples in (5, 67, 130):
                pts = tinsel_amd.gather_points(pos, nrm, samples, base_seed=17)
                mean = r.gather(pts, samples, DEPTH, mode)[:, :3].astype(np.float64)
                coef = r.gather_sh(pts, samples, DEPTH, 2, mode)
                assert (coef[..., 3].view(np.uint32) == 0).all()
                want = np.float64(Y0)*mean
                use = mean >= 1e-30
                assert use.sum() > len(pos)
                err = np.abs(coef[:, 0, :3].astype(np.float64) - want)
                bound = (2*samples + 4)*2.0**-24*np.abs(want)
                print("%s %s S=%d: largest error / bound %.3g" % (arith, mode, samples, float((err[use]/bound[use]).max())))
                assert (err[use] <= bound[use]).all(), (arith, mode, samples, float((err[use]/bound[use]).max()))
    finally:
        r.close()


# ---------------------------------------------------------------------------
# 4: the batch cut shows nowhere

@pytest.mark.parametrize("samples", [130, 5])
def test_the_batch_cut_shows_nowhere(samples):
    pos, nrm = _surface("cornell")
    n = 500                                             # (at S = 5 a batch of 1024 paths is 204 points: more than the frame gives)
    pick = np.arange(n) % len(pos)
    pts = tinsel_amd.gather_points(pos[pick], nrm[pick], samples, base_seed=7)
    assert len(np.unique(pts["seed"])) == n
    scene, r = _renderer("cornell")
    try:
        r.enable_kernel_timing(True)
        whole = r.gather_sh(pts, samples, DEPTH, 2, "sphere")
        assert r.kernel_times()["k_gather_sh_reduce"][0] == 1
        r.set_batch_paths(1024)
        per_batch = 1024//samples
        assert 1 <= per_batch < n
        cut, starts = r.gather_sh(pts, samples, DEPTH, 2, "sphere", return_starts=True)
        times = r.kernel_times()
        batches = -(-n//per_batch)
        assert times["k_gather_sh_reduce"][0] == batches and times["k_generate_gather"][0] == batches, times
    finally:
        r.close()
    assert whole.any() and np.array_equal(cut, whole)
    w1, _ = tinsel_amd.rng_state(pts["seed"][:, None] + np.arange(samples, dtype=np.uint32)[None, :], 2)
    assert np.array_equal(starts["rng1"].reshape(n, samples), w1)


# ---------------------------------------------------------------------------
# 5: the host entry across its chunk

def test_the_host_entry_across_its_chunk():
    pos, nrm = _surface("cornell")
    samples, order = 1, 2
    chunk = min(2**20, (64 << 20)//(32 + 16*9))
    assert chunk == 381300
    n = chunk + 23
    pick = np.arange(n) % len(pos)
    pts = tinsel_amd.gather_points(pos[pick], nrm[pick], samples, base_seed=11)
    assert len(np.unique(pts["seed"])) == n
    scene, r = _renderer("cornell")
    try:
        coef = r.gather_sh(pts, samples, DEPTH, order, "cosine")
        assert coef.shape == (n, 9, 4) and (coef[..., 3].view(np.uint32) == 0).all()
        # a point's coefficients are a function of its record alone: the contract on a strided subset, both sides of the cut, and the last point
        subset = np.unique(np.concatenate([np.arange(512)*(n//512), [chunk - 1, chunk, n - 1]]))
        assert len(subset) == 515 and subset[-1] == n - 1 and (subset < chunk).sum() == 513 and (subset >= chunk).sum() == 2
        sub, _ = _hold(r, pts[subset], samples, order, "cosine", "cornell cosine order 2 S=1, %d of n=%d" % (len(subset), n))
    finally:
        r.close()
    assert np.array_equal(coef[subset], sub)
    assert coef[chunk:, :, :3].any() and coef[-1, 0, :3].any()


# ---------------------------------------------------------------------------
# 6: the device entry, and what a query leaves alone

def test_the_device_entry_equals_the_host_entry_and_leaves_the_renderer_alone():
    import torch
    pos, nrm = _surface("cornell")
    n, samples = len(pos), 67
    pts = tinsel_amd.gather_points(pos, nrm, samples, base_seed=99)
    scene, r = _renderer("cornell")
    try:
        cam, opt = _cam_opt(scene)
        opt.width, opt.height = 64, 48
        r.init(64, 48)
        whole = r.render(cam, opt, passes=2).copy()
        r.init(64, 48)
        r.set_pass_index(0)
        first = r.render(cam, opt, passes=1).copy()
        before = (r.get_pass_index(), r.get_tuning().as_dict())
        host, host_starts = r.gather_sh(pts, samples, DEPTH, 2, "sphere", return_starts=True)
        s0 = r.stats()
        dev_pts = torch.from_numpy(pts.view(np.float32).reshape(n, 8).copy()).cuda()
        dev, dev_starts = r.gather_sh(dev_pts, samples, DEPTH, 2, "sphere", return_starts=True)
        assert dev.is_cuda and dev.shape == (n, 9, 4) and dev_starts.is_cuda and dev_starts.shape == (n*samples, 12)
        dev_only = r.gather_sh(dev_pts, samples, DEPTH, 1, "sphere")
        assert dev_only.shape == (n, 4, 4)
        torch.cuda.synchronize()
        s1 = r.stats()
        assert s1["samples"] - s0["samples"] == 2*n*samples and s1["rays"] - s0["rays"] >= 2*n*samples
        assert (r.get_pass_index(), r.get_tuning().as_dict()) == before and before[0] == 1
        assert r.read_accum().tobytes() == first.tobytes()
        out = r.render(cam, opt, passes=1)
        assert r.get_pass_index() == 2
    finally:
        r.close()
    assert host.any() and np.array_equal(dev.cpu().numpy(), host) and np.array_equal(dev_only.cpu().numpy(), host[:, :4])
    assert dev_starts.cpu().numpy().tobytes() == host_starts.tobytes()
    assert not np.array_equal(first, whole) and out.tobytes() == whole.tobytes()


# ---------------------------------------------------------------------------
# 7: bad arguments

def test_bad_arguments_return_minus_one_and_launch_nothing():
    pos, nrm = _surface("cornell")
    pts = tinsel_amd.gather_points(pos[:8], nrm[:8], 4)
    scene, r = _renderer("cornell")
    try:
        L, hnd = r._L, r._h
        r.enable_kernel_timing(True)
        out = np.full((8, 9, 4), 5.0, np.float32)
        starts = np.zeros(8*4, abi.PATH_START_DTYPE)
        pp, op, sp = pts.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), starts.ctypes.data_as(C.c_void_p)
        cases = {"null renderer": (None, 0, 2, 8, pp, 4, DEPTH, op, sp), "order -1": (hnd, 0, -1, 8, pp, 4, DEPTH, op, sp), "order 3": (hnd, 1, 3, 8, pp, 4, DEPTH, op, sp),
                 "mode -1": (hnd, -1, 2, 8, pp, 4, DEPTH, op, sp), "mode 2": (hnd, 2, 2, 8, pp, 4, DEPTH, op, sp),
                 "n < 0": (hnd, 0, 2, -1, pp, 4, DEPTH, op, sp), "n = 2^31": (hnd, 0, 2, 2**31, pp, 4, DEPTH, op, sp),
                 "samples 0": (hnd, 0, 2, 8, pp, 0, DEPTH, op, sp), "samples 65537": (hnd, 0, 2, 8, pp, 65537, DEPTH, op, sp),
                 "max_depth 0": (hnd, 0, 2, 8, pp, 4, 0, op, sp), "null points": (hnd, 0, 2, 8, None, 4, DEPTH, op, sp), "null out": (hnd, 0, 2, 8, pp, 4, DEPTH, None, sp),
                 "order 3, n = 0": (hnd, 0, 3, 0, None, 4, DEPTH, None, None)}
        for what, case in cases.items():
            assert L.tinsel_hip_gather_sh(*case) == -1, what
            assert L.tinsel_hip_last_error().startswith(b"gather_sh:"), what
            assert L.tinsel_hip_gather_sh_device(*case, None) == -1, what
            assert L.tinsel_hip_last_error().startswith(b"gather_sh_device:"), what
        for bad in (-1, 3):
            with pytest.raises(tinsel_amd.TinselHipError):
                r.gather_sh(pts, 4, DEPTH, bad)
        # between a move and the rebuild the scene is not in force
        last = scene.desc.num_primitives - 1
        t = abi.Transform.from_buffer_copy(bytes(C.cast(scene.desc.primitives, C.POINTER(abi.Primitive))[last].start_transform))
        t.p.x += 0.25
        r.set_primitive_transform(last, t, t)
        assert L.tinsel_hip_gather_sh(hnd, 0, 2, 8, pp, 4, DEPTH, op, sp) == -1
        msg = L.tinsel_hip_last_error()
        assert msg.startswith(b"gather_sh:") and b"call tinsel_hip_rebuild_scene first" in msg
        assert L.tinsel_hip_gather_sh_device(hnd, 0, 2, 8, pp, 4, DEPTH, op, sp, None) == -1
        assert L.tinsel_hip_last_error().startswith(b"gather_sh_device:")
        assert r.kernel_times() == {} and (out == 5.0).all() and not starts.view(np.uint32).any()
        r.rebuild_scene()
        # n == 0 is not an error, with or without arrays
        assert L.tinsel_hip_gather_sh(hnd, 0, 2, 0, None, 4, DEPTH, None, None) == 0
        assert L.tinsel_hip_gather_sh_device(hnd, 1, 0, 0, None, 4, DEPTH, None, None, None) == 0
        for order in ORDERS:
            assert r.gather_sh(pts[:0], 4, DEPTH, order).shape == (0, (order + 1)**2, 4)
        assert r.kernel_times() == {} and (out == 5.0).all()
        # and the same call with good arguments answers
        assert L.tinsel_hip_gather_sh(hnd, 0, 2, 8, pp, 4, DEPTH, op, sp) == 0
        assert (out[..., 3] == 0).all() and (out[:, 0, :3] != 5.0).all() and starts["rng1"].all()
    finally:
        r.close()


# ---------------------------------------------------------------------------
# 8: kernel times

def test_kernel_times_show_the_sh_reduction_behind_the_pipeline():
    pos, nrm = _surface("cornell")
    pts = tinsel_amd.gather_points(pos, nrm, 67)
    scene, r = _renderer("cornell")
    try:
        r.enable_kernel_timing(True)
        r.gather_sh(pts, 67, DEPTH, 2, "sphere")
        times = r.kernel_times()
        assert times["k_generate_gather"][0] == 1 and times["k_gather_sh_reduce"][0] == 1 and times["k_gather_sh_reduce"][1] > 0, times
        assert "k_gather_reduce" not in times, times
        names = list(times)
        assert names.index("k_generate_gather") < names.index("k_gather_sh_reduce")
        r.gather(pts, 67, DEPTH, "sphere")
        times = r.kernel_times()
        assert times["k_gather_reduce"][0] == 1 and "k_gather_sh_reduce" not in times, times
    finally:
        r.close()


# ---------------------------------------------------------------------------
# 9: the headless tool

def test_headless_probes_are_the_sh_gather_times_four_pi(tmp_path):
    from tinsel_amd import headless
    spp = 67
    surface, nrm = _surface("cornell")
    pick = np.arange(5)*(len(surface)//5)
    pos = (surface[pick] + np.float32(0.1)*nrm[pick]).astype(np.float32)          # five places in the room, off its surfaces
    at, path = str(tmp_path / "at.npy"), str(tmp_path / "probes.npz")
    np.save(at, pos)
    pack = os.path.join(oa.GOLDEN, "cornell.pack")
    assert headless.main(["headless", "-probes=" + path, "-probes_at=" + at, "-probes_spp=%d" % spp, "-maxdepth=%d" % DEPTH, pack]) == 0
    got = np.load(path)
    assert sorted(got.files) == ["positions", "sh"] and np.array_equal(got["positions"], pos)
    assert got["sh"].shape == (5, 9, 3) and got["sh"].dtype == np.float32
    scene, r = _renderer("cornell")
    try:
        mean = r.gather_sh(tinsel_amd.gather_points(pos, np.zeros_like(pos), spp), spp, DEPTH, 2, "sphere")
    finally:
        r.close()
    want = mean[:, :, :3]*np.float32(4.0*np.pi)
    assert want.dtype == np.float32 and want.any() and np.array_equal(got["sh"], want)
    path1 = str(tmp_path / "probes1.npz")
    assert headless.main(["headless", "-probes=" + path1, "-probes_at=" + at, "-probes_spp=%d" % spp, "-probes_order=1", "-maxdepth=%d" % DEPTH, pack]) == 0
    assert np.array_equal(np.load(path1)["sh"], want[:, :4])
    for other in ("-irradiance=i.npz", "-out=a.png", "-spp=4"):
        with pytest.raises(SystemExit, match="-probes bakes"):
            headless.main(["headless", "-probes=" + path, "-probes_at=" + at, other, pack])
    bad = str(tmp_path / "bad.npy")
    np.save(bad, np.zeros((4, 2), np.float32))
    with pytest.raises(SystemExit, match="-probes_at"):
        headless.main(["headless", "-probes=" + path, "-probes_at=" + bad, pack])

"""The feature-guided denoise stage on the GPU (tinsel_hip_denoise / _device: k_denoise_prepare, k_nlm_means, k_denoise) and
tinsel_hip_present_image_device, bit for bit.

The expected value is tests/denoise_reference.py, numpy float32 with the host libm's expf, which tests/test_denoise_abi.py pins to the
reference's NonLocalMeansFilter; the anchor below pins the kernel to that filter directly.  k_denoise works on 32 x 8 pixel tiles with a
radius-wide halo in LDS: the frames are on, one past and far inside a tile edge, narrower and lower than a tile and than the window."""
import functools
import os

import numpy as np
import pytest

import tinsel_amd
from tinsel_amd import abi
from tests import oracle_api as oa
from tests.denoise_reference import Params, denoise_reference
from tests.test_display import same_bits

pytestmark = pytest.mark.gpu
EDGE_ROWS = (21, 32, 42)        # rows of the 64 x 64 cornell frame that cross a side wall's edge (profiles/denoise_defaults.md)


def _scene(name):
    return tinsel_amd.Scene.load_pack(os.path.join(oa.GOLDEN, name + ".pack"))


@pytest.fixture(scope="module")
def renderer():
    """a renderer that is never init-ed: the stage takes caller images of any size"""
    r = tinsel_amd.create_gpu_renderer(_scene("cornell"))
    yield r
    r.close()


def _params(p):
    return tinsel_amd.denoise_params(**{k: getattr(p, k) for k in ("radius", "patch_radius", "k_color", "k_albedo", "k_normal", "k_depth", "demodulate",
                                                                  "albedo_floor")})


# ---------------------------------------------------------------------------
# 1: the anchor -- with the guide terms off the kernel is the reference's NonLocalMeansFilter

@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("shape", [(21, 37), (3, 5)])
def test_without_guides_the_device_entry_is_the_reference_nlm(renderer, shape, radius):
    import torch
    rng = np.random.default_rng(7*radius + shape[0])
    P = oa.PortOracle()
    c = rng.random(shape + (3,)).astype(np.float32)
    image = np.zeros(shape + (4,), np.float32)
    image[..., :3] = c
    beauty = np.ones(shape + (4,), np.float32)
    beauty[..., :3] = c
    for falloff in (200.0, 3.0):
        want = P.nlm(image, falloff, radius)
        got = renderer.denoise(None, _params(Params(radius, radius, falloff)), beauty=torch.from_numpy(beauty).cuda())
        assert isinstance(got, torch.Tensor) and got.is_cuda
        got = got.cpu().numpy()
        assert same_bits(got[..., :3], want[..., :3]) and (got[..., 3] == 1.0).all()


# ---------------------------------------------------------------------------
# 2: the full statement on synthetic planes

@functools.lru_cache(maxsize=None)
def _synthetic(H, W):
    """(beauty, planes [3, H, W, 4]): random, with a block of pixels without weight, a block of misses, albedo channels under the floor"""
    rng = np.random.default_rng(1000*H + W)
    f = lambda *s: rng.random(s).astype(np.float32)
    beauty = f(H, W, 4)*np.float32(2.0)
    beauty[..., 3] += np.float32(0.25)
    albedo, normal, depth = f(H, W, 4), f(H, W, 4)*np.float32(2.0) - np.float32(1.0), f(H, W, 4)
    for plane in (albedo, normal, depth):
        plane[..., 3] = beauty[..., 3]
    depth[..., 0] = depth[..., 2]*(np.float32(1.0) + np.float32(9.0)*f(H, W))            # mean depth 1 .. 10
    albedo[..., :3] *= albedo[..., 3:4]
    y0, y1, x0, x1 = H//4, max(H//4 + 1, H//2), W//5, max(W//5 + 1, W//2)
    beauty[y0:y1, x0:x1, 3] = 0.0                                                         # no weight (the sums are left as they are)
    for plane in (albedo, normal, depth):
        plane[y0:y1, x0:x1, 3] = 0.0
    my0, mx0 = H//2, W//2
    depth[my0:, mx0:, :3] = 0.0                                                           # misses: D.z == 0, albedo 0
    albedo[my0:, mx0:, :3] = 0.0
    normal[my0:, mx0:, :3] = 0.0
    albedo[::3, 1::2, 1] *= np.float32(0.01)                                              # under the floor
    albedo[1::4, ::3, :3] *= np.float32(0.02)
    planes = np.stack([albedo, normal, depth])
    beauty.setflags(write=False)
    planes.setflags(write=False)
    return beauty, planes


def _case(shape, radius, patch, mask, demodulate):
    return pytest.param(shape, radius, patch, mask, demodulate, id="%dx%d-r%d-p%d-m%d-d%d" % (shape[1], shape[0], radius, patch, mask, demodulate))


CASES = [_case((21, 37), r, 1, 7, 1) for r in (1, 3, 8)] + \
        [_case(s, 8, 4, 7, 1) for s in ((3, 5), (1, 1))] + \
        [_case(s, 3, 0, 7, 0) for s in ((16, 16), (33, 17), (8, 32), (9, 33), (17, 65))] + \
        [_case((21, 37), 3, p, 7, 1) for p in (0, 4)] + \
        [_case((21, 37), 3, 1, m, d) for m in range(8) for d in ((0, 1) if m & 1 else (0,)) if (m, d) != (7, 1)]


@pytest.mark.parametrize("shape,radius,patch,mask,demodulate", CASES)
def test_the_host_entry_is_the_statement_on_synthetic_planes(renderer, shape, radius, patch, mask, demodulate):
    beauty, planes = _synthetic(*shape)
    names = [n for k, n in enumerate(abi.FEATURE_NAMES) if mask >> k & 1]
    given = {n: planes[abi.FEATURE_NAMES.index(n)] for n in names}
    p = Params(radius, patch, 2.0, 3.0, 1.5, 4.0, demodulate, 0.05)
    want = denoise_reference(beauty, [given[n] for n in names], mask, p)
    got = renderer.denoise(given, _params(p), beauty=beauty)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.isfinite(want).all()
    bad = (got.view(np.uint32) != want.view(np.uint32)).any(axis=-1)
    assert not bad.any(), "%d of %d pixels differ (first: row %d column %d, %s against %s)" % (
        int(bad.sum()), bad.size, *np.unravel_index(np.argmax(bad), bad.shape), got[np.unravel_index(np.argmax(bad), bad.shape)],
        want[np.unravel_index(np.argmax(bad), bad.shape)])


def test_the_guides_and_the_demodulation_change_the_result(renderer):
    """(the cases above would also pass if every mask ran the same kernel on the same numbers)"""
    beauty, planes = _synthetic(21, 37)
    p = _params(Params(3, 1, 2.0, 3.0, 1.5, 4.0, 0, 0.05))
    seen = []
    for mask in range(8):
        given = {n: planes[k] for k, n in enumerate(abi.FEATURE_NAMES) if mask >> k & 1}
        seen.append(renderer.denoise(given, p, beauty=beauty).tobytes())
    given = {n: planes[k] for k, n in enumerate(abi.FEATURE_NAMES)}
    seen.append(renderer.denoise(given, _params(Params(3, 1, 2.0, 3.0, 1.5, 4.0, 1, 0.05)), beauty=beauty).tobytes())
    assert len(set(seen)) == 9


# ---------------------------------------------------------------------------
# 3: end to end on the renderer's own accumulator and features

def test_end_to_end_on_the_accumulator_and_its_features():
    import torch
    W, H, SPP = 96, 64, 8
    scene = _scene("features_probe")
    r = tinsel_amd.create_gpu_renderer(scene)
    try:
        cam, opt = scene.camera, scene.options.copy()
        opt.width, opt.height = W, H
        r.init(W, H)
        r.render(cam, opt, passes=SPP, readback=False)
        accum, index, stats = r.read_accum(), r.get_pass_index(), r.stats()
        planes = r.features(cam, opt, 0, SPP)
        p = tinsel_amd.denoise_params()
        want = denoise_reference(accum, [planes[n] for n in abi.FEATURE_NAMES], 7, p)
        got = r.denoise(planes)
        assert same_bits(got, want) and np.isfinite(got).all()
        # the device path: the planes and the result stay on the device
        t = torch.empty((3, H, W, 4), dtype=torch.float32, device="cuda:0")
        planes_dev = r.features(cam, opt, 0, SPP, out=t)
        got_dev = r.denoise(planes_dev)
        assert isinstance(got_dev, torch.Tensor) and got_dev.is_cuda
        assert np.array_equal(got_dev.cpu().numpy().view(np.uint32), got.view(np.uint32))
        # ... with the beauty given as a tensor, into a tensor of the caller's, planes that are not neighbours
        out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
        apart = {n: v.clone() for n, v in planes_dev.items()}
        assert r.denoise(apart, beauty=torch.from_numpy(accum).cuda(), out=out) is out
        assert np.array_equal(out.cpu().numpy().view(np.uint32), got.view(np.uint32))
        # nothing of the renderer's moved
        assert np.array_equal(r.read_accum().view(np.uint32), accum.view(np.uint32))
        assert r.get_pass_index() == index and r.stats() == stats
        # a refusal reaches the caller as the library words it
        with pytest.raises(tinsel_amd.TinselHipError, match="denoise"):
            r.denoise(planes, beauty=None, params=tinsel_amd.denoise_params(radius=9))
    finally:
        r.close()


# ---------------------------------------------------------------------------
# 4: the display stage on an image of the caller's

def test_present_image_is_present_on_a_copy_and_the_reference_display_on_the_denoised_image():
    import torch
    W, H, SPP = 96, 64, 8
    scene = _scene("features_probe")
    r = tinsel_amd.create_gpu_renderer(scene)
    try:
        cam, opt = scene.camera, scene.options.copy()
        opt.width, opt.height, opt.exposure = W, H, 1.3
        r.init(W, H)
        accum = r.render(cam, opt, passes=SPP)
        copy = torch.from_numpy(accum).cuda()
        for nlm in ((0, 200.0), (1, 200.0), (2, 50.0)):
            want = r.present(opt, *nlm)
            got = r.present_image(copy, opt, *nlm)
            assert isinstance(got, torch.Tensor) and same_bits(got.cpu().numpy(), want), nlm
            assert same_bits(r.present_image(accum, opt, *nlm), want), nlm                     # a numpy image: uploaded, numpy back
            assert same_bits(r.present(opt, *nlm), want), nlm                                   # present itself is as it was
        denoised = r.denoise(r.features(cam, opt, 0, SPP))
        P = oa.PortOracle()
        want = P.present(denoised, opt.exposure, opt.limit)
        assert same_bits(r.present_image(denoised, opt), want)
        assert same_bits(r.present_image(torch.from_numpy(denoised).cuda(), opt).cpu().numpy(), want)
        assert same_bits(r.present_image(denoised, opt, 1, 200.0), P.nlm(want, 200.0, 1))
    finally:
        r.close()


# ---------------------------------------------------------------------------
# 5: it denoises

def test_it_denoises_cornell_and_keeps_the_wall_edge_in_place():
    """Cornell at 64 x 64 and 4 spp with the defaults, against 1024 spp by the same renderer: a lower mean squared error than the noisy
    frame, and along rows that cross the edge between two walls -- the largest horizontal step of the albedo plane -- the steepest
    horizontal step of the radiance within 4 columns of it falls in the same pixel as in the 1024-spp image.
    (profiles/denoise_defaults.md: the host statement meets both on the reference's own renders.)"""
    W = H = 64
    scene = _scene("cornell")
    r = tinsel_amd.create_gpu_renderer(scene)
    try:
        cam, opt = scene.camera, scene.options.copy()
        opt.width, opt.height = W, H
        r.init(W, H)
        noisy = r.render(cam, opt, passes=4).copy()
        planes = r.features(cam, opt, 0, 4)
        denoised = r.denoise(planes)
        r.init(W, H)
        r.set_pass_index(0)
        clean = r.render(cam, opt, passes=1024)
    finally:
        r.close()
    colour = lambda a: (a[..., :3].astype(np.float64)/a[..., 3:4])
    mse = lambda a, b: float(np.mean((a - b)**2))
    clean, before, after = colour(clean), colour(noisy), colour(denoised)
    print("mse against 1024 spp: noisy %.6f, denoised %.6f" % (mse(before, clean), mse(after, clean)))
    assert mse(after, clean) < mse(before, clean)
    albedo = colour(planes["albedo"])
    for row in EDGE_ROWS:
        x = int(np.argmax(np.abs(np.diff(albedo[row], axis=0)).sum(axis=1)))
        lo, hi = max(0, x - 4), min(W - 1, x + 5)
        step = lambda im: lo + int(np.argmax(np.abs(np.diff(im[row], axis=0)).sum(axis=1)[lo:hi]))
        print("row %d: albedo edge at column %d, steepest step: 1024 spp %d, denoised %d" % (row, x, step(clean), step(after)))
        assert step(after) == step(clean), row


# ---------------------------------------------------------------------------
# 6: the headless option

def test_headless_denoise_writes_the_presented_denoised_frame(tmp_path):
    from tinsel_amd import headless
    from tinsel_amd.display import png_bytes, quantize_rgb8
    W, H, SPP = 48, 32, 4
    pack = os.path.join(oa.GOLDEN, "cornell.pack")
    out = tmp_path / "d.png"
    assert headless.main(["headless", "-denoise=3", "-spp=%d" % SPP, "-width=%d" % W, "-height=%d" % H, "-out=%s" % out, pack]) == 0
    scene = _scene("cornell")
    r = tinsel_amd.create_gpu_renderer(scene)
    try:
        cam, opt = scene.camera, scene.options.copy()
        opt.width, opt.height, opt.max_samples = W, H, SPP
        r.init(W, H)
        r.render(cam, opt, passes=SPP, readback=False)
        plain = r.present(opt)
        image = r.present_image(r.denoise(r.features(cam, opt, 0, SPP), tinsel_amd.denoise_params(radius=3)), opt)
    finally:
        r.close()
    data = open(out, "rb").read()
    assert data == png_bytes(quantize_rgb8(image)) and data != png_bytes(quantize_rgb8(plain))

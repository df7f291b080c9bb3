"""k_accumulate_tiled's support form (tinsel_amd/csrc/tn_accumulate.h) against its full-window form and against AddSample, through
tinsel_hip_selftest_accumulate: the launch a render makes, on radiance the test chooses.  Every comparison is of every bit: the support form
skips nothing but adds of +0, and where such an add is no no-op (a non-finite sample, a -0 in the accumulator) it has to notice.

The reference is tests/accumulate_reference.py (AddSample over whole passes in numpy float32; tests/test_accumulate_support.py holds it to
the oracle's own framebuffer).  The hook renders one shard; a shard's tile list goes through tests/test_gpu_parity.py's sharded renders."""
import numpy as np
import pytest

import tinsel_amd
from tinsel_amd import abi
from tests.accumulate_reference import F, add_passes, raster_draws
from tests.test_accumulate_support import FILTERS

pytestmark = pytest.mark.gpu

FRAMES = [(1, 1), (1, 40), (17, 16), (33, 19), (64, 64)]        # (width, height): one pixel, one column, a tile and a bit, 3 x 2 tiles, 16 whole tiles
NO_CLAMP = float(np.finfo(np.float32).max)
SUPPORT_RAN = {abi.ACCUMULATE_TILED: abi.ACCUMULATE_RAN_SUPPORT_TILED, abi.ACCUMULATE_WIDE: abi.ACCUMULATE_RAN_SUPPORT_WIDE}
FULL_RAN = {abi.ACCUMULATE_TILED: abi.ACCUMULATE_RAN_TILED, abi.ACCUMULATE_WIDE: abi.ACCUMULATE_RAN_WIDE}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _seed_where(pred, start=1):
    """the first seed from `start` on whose draws for pixel (0, 0) satisfy pred(x, y)"""
    for seed in range(start, start + 100000):
        x, y = raster_draws(1, 1, seed)
        if pred(float(x[0, 0]), float(y[0, 0])):
            return seed
    raise AssertionError("no such seed")


def _seeds(W, H, passes):
    """Seeds whose draws fall below 0.25, above 0.75 and in the bands around both, per axis: picked for the one-pixel frame, checked for all"""
    if W*H == 1:
        picks = [_seed_where(lambda x, y: x < 0.25 and y > 0.75), _seed_where(lambda x, y: abs(x - 0.25) < 0.004 and abs(y - 0.75) < 0.05),
                 _seed_where(lambda x, y: x > 0.75 and abs(y - 0.25) < 0.05)]
        return picks[:passes] if passes < 3 else picks
    seeds = [0x9e3779b9 + 7919*s for s in range(passes)]
    if W*H >= 256:
        for s in seeds[:1]:
            for d in raster_draws(W, H, s):
                assert (d < 0.25).any() and (d > 0.75).any() and (abs(d - 0.25) < 0.01).any() and (abs(d - 0.75) < 0.01).any()
    return seeds


def _radiance(W, H, passes, seed):
    rng = np.random.default_rng(seed)
    rad = (rng.random((passes, H, W, 4))*8.0).astype(np.float32)           # up to 8 per channel: a clamp of 4 bites
    rad[rng.random((passes, H, W)) < 0.1] = 0.0                             # black paths
    return rad


def _accum(W, H, seed):
    return np.random.default_rng(seed).random((H, W, 4)).astype(np.float32)


def _not_finite(rad):
    """rad[3, H, W, 4] with an inf, a NaN or a -inf component at five spots (a frame's corners, both sides of a tile's edge) and one huge finite
    sample; returns it and the (pass, row, column) of the spots"""
    H, W = rad.shape[1:3]
    spots = [(0, 0, 0), (1, min(H - 1, 15), min(W - 1, 16)), (2, H - 1, W - 1), (1, H//2, min(W - 1, 15)), (0, min(H - 1, 16), min(W - 1, 3))]
    for n, (s, j, i) in enumerate(spots):
        rad[s, j, i, n % 3] = [np.inf, np.nan, -np.inf][n % 3]
    rad[2, min(H - 1, 1), min(W - 1, 1), :3] = 3.0e38
    return rad, spots


def _check_forms(rad, acc0, seeds, filt, clamp, equal_nan=False):
    """full window == AddSample, support == full window bit for bit, for both workgroup sizes; returns the result"""
    want = add_passes(acc0, rad, seeds, filt, clamp)
    for choice in (abi.ACCUMULATE_TILED, abi.ACCUMULATE_WIDE):
        full, ran = tinsel_amd.selftest_accumulate(rad, acc0, seeds, filt, clamp, choice, abi.ACCUMULATE_FORM_FULL_WINDOW)
        assert ran == FULL_RAN[choice]
        sup, ran = tinsel_amd.selftest_accumulate(rad, acc0, seeds, filt, clamp, choice, abi.ACCUMULATE_FORM_SUPPORT)
        assert ran == SUPPORT_RAN[choice]
        auto, ran = tinsel_amd.selftest_accumulate(rad, acc0, seeds, filt, clamp, choice, abi.ACCUMULATE_FORM_AUTO)
        assert ran == SUPPORT_RAN[choice]
        if equal_nan:       # (the sign of the NaN an invalid operation makes is the processor's: x86 sets it, the GPU does not)
            assert np.array_equal(full, want, equal_nan=True) and np.array_equal(np.isnan(full), np.isnan(want))
        else:
            assert np.array_equal(_bits(full), _bits(want))
        assert np.array_equal(_bits(sup), _bits(full)) and np.array_equal(_bits(auto), _bits(full))
    return want


@pytest.mark.parametrize("passes", [1, 3])
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: "%dx%d" % f)
@pytest.mark.parametrize("name", ["cornell", "default", "half"])
def test_the_support_form_adds_what_the_full_window_adds(name, frame, passes):
    W, H = frame
    filt, takes = FILTERS[name]
    assert takes
    seeds = _seeds(W, H, passes)
    for clamp in (4.0, NO_CLAMP):
        _check_forms(_radiance(W, H, passes, W*1000 + H), _accum(W, H, 5), seeds, filt, clamp)
    # a render's first batch: the accumulator all +0
    _check_forms(_radiance(W, H, passes, 11), np.zeros((H, W, 4), np.float32), seeds, filt, 4.0)


@pytest.mark.parametrize("passes", [1, 3])
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: "%dx%d" % f)
@pytest.mark.parametrize("name", ["one", "box", "offset0", "wide"])
def test_other_filters_keep_the_full_window(name, frame, passes):
    """the borderline Gaussian (zero radius exactly 1), the box, a Gaussian without offset, a width beyond 1: today's kernels, today's adds"""
    W, H = frame
    filt, takes = FILTERS[name]
    assert not takes
    seeds = _seeds(W, H, passes)
    rad, acc0 = _radiance(W, H, passes, 3), _accum(W, H, 4)
    want = add_passes(acc0, rad, seeds, filt, 4.0)
    for choice, ran_want in ((abi.ACCUMULATE_TILED, abi.ACCUMULATE_RAN_TILED), (abi.ACCUMULATE_WIDE, abi.ACCUMULATE_RAN_WIDE if name != "wide" else abi.ACCUMULATE_RAN_TILED)):
        got, ran = tinsel_amd.selftest_accumulate(rad, acc0, seeds, filt, 4.0, choice, abi.ACCUMULATE_FORM_AUTO)
        assert ran == ran_want
        assert np.array_equal(_bits(got), _bits(want))
        with pytest.raises(tinsel_amd.TinselHipError):
            tinsel_amd.selftest_accumulate(rad, acc0, seeds, filt, 4.0, choice, abi.ACCUMULATE_FORM_SUPPORT)


@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: "%dx%d" % f)
def test_what_a_render_launches(frame):
    """AUTO as launch_accumulate resolves it for such a frame: few tiles go to k_accumulate_piped, which has no support form and needs none;
    TINSEL_ACCUMULATE_FULL_WINDOW is AUTO without the support form"""
    W, H = frame
    filt = FILTERS["cornell"][0]
    seeds = _seeds(W, H, 3)
    rad, acc0 = _radiance(W, H, 3, 8), _accum(W, H, 9)
    want = add_passes(acc0, rad, seeds, filt, NO_CLAMP)
    for choice in (abi.ACCUMULATE_AUTO, abi.ACCUMULATE_FULL_WINDOW, abi.ACCUMULATE_PIPED):
        got, ran = tinsel_amd.selftest_accumulate(rad, acc0, seeds, filt, NO_CLAMP, choice, abi.ACCUMULATE_FORM_AUTO)
        assert ran == abi.ACCUMULATE_RAN_PIPED         # (at most 16 tiles: a block per CU or less)
        assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("frame", [(17, 16), (33, 19), (64, 64)], ids=lambda f: "%dx%d" % f)
@pytest.mark.parametrize("name", ["cornell", "default"])
def test_samples_that_are_not_finite_go_through_the_full_window(name, frame):
    """0*inf is NaN: a sample with an infinite or NaN component reaches every pixel of its footprint in the reference, also those its weight is
    +0 for -- in its own tile and, from the first pixel beyond a tile's edge, in the neighbouring one.  A huge finite sample with the clamp off
    (its length overflows: ClampLength scales it to 0) does not."""
    W, H = frame
    filt = FILTERS[name][0]
    seeds = _seeds(W, H, 3)
    rad, _ = _not_finite(_radiance(W, H, 3, 21))
    for clamp in (4.0, NO_CLAMP):
        want = _check_forms(rad, _accum(W, H, 6), seeds, filt, clamp, equal_nan=True)
        assert np.isnan(want).any() and np.isfinite(want[..., 3]).all()
        if name == "cornell":       # the whole 3 x 3 footprint of the interior inf sample is NaN, not only the 2 x 2 pixels its weight is non-zero for
            assert np.isnan(want[..., 0]).sum() >= 9


@pytest.mark.parametrize("frame", [(1, 1), (17, 16), (33, 19)], ids=lambda f: "%dx%d" % f)
def test_a_negative_zero_in_the_accumulator_keeps_the_full_window(frame):
    """-0 + +0 is +0: where the accumulator holds a -0, an add of +0 the support form would skip changes a bit"""
    W, H = frame
    filt = FILTERS["cornell"][0]
    seeds = _seeds(W, H, 3)
    acc0 = _accum(W, H, 12)
    acc0[::2, ::3] = -0.0
    acc0[H - 1, W - 1, 1] = -0.0
    rad = _radiance(W, H, 3, 13)
    rad[:, ::2, ::3] = 0.0                  # (black paths over the -0 pixels, so that some stay zero)
    want = _check_forms(rad, acc0, seeds, filt, 4.0)
    if W*H > 1:
        assert (_bits(want) == 0).any()     # a -0 that became +0 ...
    # ... and an accumulator of -0 under black paths everywhere: every -0 a sample reaches turns +0
    _check_forms(np.zeros_like(rad), np.full((H, W, 4), -0.0, np.float32), seeds, filt, 4.0)


@pytest.mark.parametrize("frame", [(17, 16), (33, 19)], ids=lambda f: "%dx%d" % f)
def test_negative_samples(frame):
    """x + (-0) is x: negative radiance (and its -0 products with a +0 weight) needs no guard"""
    W, H = frame
    seeds = _seeds(W, H, 3)
    rad = _radiance(W, H, 3, 31) - 4.0
    for name in ("cornell", "half"):
        _check_forms(rad, _accum(W, H, 32) - 0.5, seeds, FILTERS[name][0], NO_CLAMP)
        _check_forms(rad, np.zeros((H, W, 4), np.float32), seeds, FILTERS[name][0], 4.0)


FULL_WINDOW_RUNS = [(abi.ACCUMULATE_TILED, abi.ACCUMULATE_FORM_FULL_WINDOW, abi.ACCUMULATE_RAN_TILED),
                    (abi.ACCUMULATE_WIDE, abi.ACCUMULATE_FORM_FULL_WINDOW, abi.ACCUMULATE_RAN_WIDE),
                    (abi.ACCUMULATE_PIPED, abi.ACCUMULATE_FORM_FULL_WINDOW, abi.ACCUMULATE_RAN_PIPED),
                    (abi.ACCUMULATE_AUTO, abi.ACCUMULATE_FORM_AUTO, abi.ACCUMULATE_RAN_PIPED)]      # (a handful of tiles: a block per CU or less)


@pytest.mark.parametrize("frame", [(1, 1), (17, 16), (33, 19)], ids=lambda f: "%dx%d" % f)
@pytest.mark.parametrize("name", ["cornell", "default", "one", "box"])
def test_every_full_window_kernel_adds_the_same_whatever_the_samples(name, frame):
    """The full window of k_accumulate_tiled at both workgroup sizes and k_accumulate_piped (which the tests above reach with finite samples
    and one filter only) stage and add with the same arithmetic: samples that are not finite, an accumulator with -0 entries, the Gaussian
    of both compile-time windows, the borderline Gaussian and the box.  GPU against GPU every bit compares, the sign of a NaN too; against
    AddSample every bit of every number, and the same components NaN (the sign of the NaN an invalid operation makes is the processor's)."""
    W, H = frame
    filt = FILTERS[name][0]
    seeds = _seeds(W, H, 3)
    rad, spots = _not_finite(_radiance(W, H, 3, 41))
    acc0 = _accum(W, H, 42)
    acc0[::2, ::3] = -0.0
    acc0[H - 1, W - 1, 1] = -0.0
    near = np.zeros((H, W), bool)           # what a sample generated at a spot can reach: at most two pixels away (filter widths up to 1)
    for _, j, i in spots:
        near[max(0, j - 2):j + 3, max(0, i - 2):i + 3] = True
    for clamp in (4.0, NO_CLAMP):
        want = add_passes(acc0, rad, seeds, filt, clamp)
        nan = np.isnan(want)
        assert nan.any() and not nan[~near].any()
        got = []
        for choice, form, ran_want in FULL_WINDOW_RUNS:
            out, ran = tinsel_amd.selftest_accumulate(rad, acc0, seeds, filt, clamp, choice, form)
            assert ran == ran_want
            got.append(out)
        for out in got:
            assert np.array_equal(_bits(out), _bits(got[0]))
        assert np.array_equal(np.isnan(got[0]), nan) and np.array_equal(_bits(got[0])[~nan], _bits(want)[~nan])

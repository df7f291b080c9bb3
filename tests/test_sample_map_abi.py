"""Sample maps without a GPU: the three symbols and the refusals that need no device, the batch cut tinsel_hip_plan_sample_map states
against a few lines of Python, the crop helper, and the yardstick of the GPU tests (tests/sample_map_reference.py) held to the oracle: its
masked statement with a full mask IS accumulate_reference.add_passes IS the oracle's accumulator, and the chaining identity holds bit for
bit.  The oracle here is the plain-C port, which every machine builds."""
import ctypes as C

import numpy as np
import pytest

import tinsel_amd
from tinsel_amd import abi
from tests import accumulate_reference as ar
from tests import oracle_api as oa
from tests import sample_map_reference as sm

W, H, LEVELS = sm.W, sm.H, 5


# ---------------------------------------------------------------------------
# the symbols

def test_the_symbols_and_the_refusals_that_need_no_device():
    L = tinsel_amd.load_library()
    for name in ("tinsel_hip_render_sample_map", "tinsel_hip_render_sample_map_device", "tinsel_hip_plan_sample_map"):
        assert hasattr(L, name) and name in tinsel_amd.renderer.EXPORTED_SYMBOLS, name
    assert abi.SAMPLE_MAP_MAX == 65535 == np.iinfo(np.uint16).max and abi.SAMPLES_ADD == 1
    cam, opt = sm.frame("cornell")
    counts = np.ones((H, W), np.uint16)
    out = np.full((H, W, 4), 7.0, np.float32)
    cp, op = counts.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    # no renderer: refused before anything is read or written
    assert L.tinsel_hip_render_sample_map(None, C.byref(cam), C.byref(opt), 0, cp, 0, op) == -1
    assert b"null argument" in L.tinsel_hip_last_error()
    assert L.tinsel_hip_render_sample_map_device(None, C.byref(cam), C.byref(opt), 0, cp, 0, op, None) == -1
    assert b"null argument" in L.tinsel_hip_last_error()
    assert (out == 7.0).all()
    with pytest.raises(ValueError):
        tinsel_amd.plan_sample_map(1 << 20, W, H, counts.astype(np.int32))         # uint16 only
    with pytest.raises(ValueError):
        tinsel_amd.plan_sample_map(1 << 20, W, H, counts.T)


# ---------------------------------------------------------------------------
# tinsel_hip_plan_sample_map

def _maps():
    tall = np.zeros((H, W), np.uint16)
    tall[7, 11] = 40
    tall[::3, ::2] = 1
    return {"uniform_5": np.full((H, W), 5, np.uint16), "random": sm.random_counts(3), "zero": np.zeros((H, W), np.uint16), "tall": tall,
            "most": np.full((H, W), 65535, np.uint16)}


PLAN_CASES = {
    # limit, map, (levels per batch, batches, paths, largest count)
    "everything_fits": (64 << 20, "uniform_5", (69905, 1, 5*W*H, 5)),
    "a_limit_below_one_level": (100, "uniform_5", (1, 5, 5*W*H, 5)),
    "a_limit_of_nothing": (0, "random", (1, 5, None, 5)),
    "exactly_two_levels": (2*W*H, "uniform_5", (2, 3, 5*W*H, 5)),
    "one_slot_short_of_two_levels": (2*W*H - 1, "uniform_5", (1, 5, 5*W*H, 5)),
    "exactly_the_map's_levels": (5*W*H, "random", (5, 1, None, 5)),
    "an_all_zero_map": (1024, "zero", (1, 0, 0, 0)),
    "one_tall_pixel": (8*W*H, "tall", (8, 5, None, 40)),
    "a_limit_beyond_32_bits": (1 << 40, "most", ((2**32 - 2)//(W*H), 1, 65535*W*H, 65535)),
}


@pytest.mark.parametrize("case", sorted(PLAN_CASES))
def test_plan_sample_map_states_the_cut(case):
    limit, which, want = PLAN_CASES[case]
    counts = _maps()[which]
    got = tinsel_amd.plan_sample_map(limit, W, H, counts)
    rule = sm.plan(limit, W, H, counts)
    assert got == rule, (case, got, rule)
    assert all(w is None or w == g for w, g in zip(want, got)), (case, got)
    levels, batches, paths, most = got
    assert levels >= 1 and levels*W*H < 2**32 - 1                   # one level at least; no batch has 2^32 - 1 slots or more
    assert levels*W*H <= max(limit, W*H)                            # under the limit, but for a single level larger than it
    # the batches' offsets: compact, and their path counts add up to the map's
    total = 0
    for b in range(batches):
        off = sm.batch_offsets(counts, b*levels, levels)
        assert off[0] == 0 and len(off) == W*H + 1 and (np.diff(off) >= 0).all() and np.diff(off).max() <= levels
        assert 0 < off[-1] <= levels*W*H                            # a batch below the largest count is never empty
        total += int(off[-1])
    assert total == paths == int(counts.astype(np.int64).sum())


def test_plan_sample_map_over_a_sweep_and_its_refusals():
    rng = np.random.RandomState(7)
    for _ in range(200):
        width, height = int(rng.randint(1, 70)), int(rng.randint(1, 70))
        counts = rng.randint(0, int(rng.choice([1, 2, 6, 300, 65536])), (height, width)).astype(np.uint16)
        limit = int(2**rng.uniform(0, 34))
        assert tinsel_amd.plan_sample_map(limit, width, height, counts) == sm.plan(limit, width, height, counts)
    L = tinsel_amd.load_library()
    out = (C.c_ulonglong*4)()
    one = np.ones(1, np.uint16).ctypes.data_as(C.c_void_p)
    for args in ((1 << 20, 0, 24, one), (1 << 20, 40, 0, one), (1 << 20, 40, 24, None)):
        assert L.tinsel_hip_plan_sample_map(*args, out) == -1 and L.tinsel_hip_last_error()
    assert L.tinsel_hip_plan_sample_map(1 << 20, 1, 1, one, None) == -1
    # the 2^32 - 1 bound: one level of the frame is the smallest batch there is (the counts are not read)
    assert sm.plan(1 << 20, 65536, 65536, np.ones(1)) is None
    assert L.tinsel_hip_plan_sample_map(1 << 20, 65536, 65536, one, out) == -1 and b"32-bit" in L.tinsel_hip_last_error()
    assert L.tinsel_hip_plan_sample_map(1 << 20, 65535, 65537, one, out) == -1          # 2^32 - 1 exactly
    assert L.tinsel_hip_plan_sample_map(1 << 20, 2, 1, np.array([3, 1], np.uint16).ctypes.data_as(C.c_void_p), out) == 0 and tuple(out) == (524288, 1, 4, 3)


def test_crop_sample_map():
    c = tinsel_amd.crop_sample_map(W, H, 5, 3, 27, 19, 4)
    assert c.dtype == np.uint16 and c.shape == (H, W) and c.sum() == 4*22*16
    assert (c[3:19, 5:27] == 4).all() and not c[:3].any() and not c[19:].any() and not c[:, :5].any() and not c[:, 27:].any()
    assert np.array_equal(tinsel_amd.crop_sample_map(W, H, -3, -2, W + 9, H + 1, 2), np.full((H, W), 2, np.uint16))     # cut to the frame
    assert not tinsel_amd.crop_sample_map(W, H, 9, 9, 9, 12, 2).any() and not tinsel_amd.crop_sample_map(W, H, 12, 9, 9, 12, 2).any()
    with pytest.raises(ValueError):
        tinsel_amd.crop_sample_map(W, H, 0, 0, 4, 4, 65536)


# ---------------------------------------------------------------------------
# the yardstick against the oracle (the plain-C port)

def _port_levels(name, pass_begin, levels):
    O = oa.PortOracle()
    cam, opt = sm.frame(name)
    h = O.load_pack(sm.pack_bytes(name))
    try:
        accum, rad, _ = O.render_seeded(h, cam, opt, pass_begin, levels, threads=4, want_radiance=True)
        seeds = [int(O.pass_seed(pass_begin + t)) & 0xffffffff for t in range(levels)]
    finally:
        O.free(h)
    return opt, accum, rad, seeds


@pytest.mark.skipif(not oa.have_port(), reason="oracle/libtinsel_oracle.so is not built")
@pytest.mark.parametrize("name", ["cornell", "veach", "motionblur"])
def test_the_masked_statement_against_the_oracle(name):
    opt, accum, rad, seeds = _port_levels(name, 0, LEVELS)
    assert name != "veach" or opt.clamp == 4.0
    filt, zero = sm.filter_of(opt), np.zeros((H, W, 4), np.float32)
    # add_passes on the oracle's radiance is the oracle's accumulator; the masked form with a full mask is add_passes
    full = ar.add_passes(zero, rad, seeds, filt, opt.clamp)
    assert np.array_equal(full, accum) and accum[..., :3].any()
    assert np.array_equal(sm.add_levels(zero, rad, seeds, filt, opt.clamp, np.ones((LEVELS, H, W), bool)), full)
    # a random map in 0 .. 5: finite, and not the full frame
    counts = sm.random_counts(11)
    assert (counts == 0).any() and (counts == LEVELS).any()
    masked = sm.add_levels(zero, rad, seeds, filt, opt.clamp, sm.live_levels(counts))
    assert np.isfinite(masked).all() and not np.array_equal(masked, full)
    # a skipped sample is not a black one: the weight channel is smaller wherever a neighbour is short of samples
    assert (masked[..., 3] <= full[..., 3]).all() and (masked[..., 3] < full[..., 3]).any()
    # chaining: a uniform `a` levels, then the map c at level a on top of it, is the single map a + c
    a = 2
    c = np.minimum(counts, LEVELS - a).astype(np.uint16)
    first = sm.add_levels(zero, rad[:a], seeds[:a], filt, opt.clamp, np.ones((a, H, W), bool))
    assert np.array_equal(first, ar.add_passes(zero, rad[:a], seeds[:a], filt, opt.clamp))
    chained = sm.add_levels(first, rad[a:], seeds[a:], filt, opt.clamp, sm.live_levels(c)) if c.any() else first
    assert np.array_equal(chained, sm.add_levels(zero, rad, seeds, filt, opt.clamp, sm.live_levels(a + c)))

"""The support form of k_accumulate_tiled (tinsel_amd/csrc/tn_accumulate.h) rests on host arithmetic that needs no GPU to check:

  - Filter::Gaussian is max(0, expf(a) - offset) with a = -falloff*x*x.  For a <= argZero = log(offset) - 1e-6 (double, rounded down to float)
    the float expf(a) is at most `offset`, so the weight is +0: checked on the host's expf (which the device's restates bit for bit,
    tests/test_gpu_leaf.py) over the 2^17 floats at and below argZero and over 10^5 random arguments down to -falloff*9;
  - launch_accumulate's rule: which filters take the support form (tinsel_hip_accumulate_support, the library's own host function, and its
    restatement in tinsel_amd/abi.py);
  - tests/accumulate_reference.py, the numpy AddSample the GPU test compares with, against the oracle's own framebuffer."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import tinsel_amd
from tinsel_amd import abi
from tests.accumulate_reference import F, add_passes, constructor_offset, expf
from tests.oracle_api import GOLDEN, PortOracle, RefOracle, have_port, have_ref

CORNELL_OFFSET = constructor_offset(0.75, 1.0)          # the reference's main.cpp constructs Filter(gaussian, 0.75, 1.0); the scene's `filter` line keeps that offset
FILTERS = {                                             # name: (type, width, falloff, offset), takes the support form?
    "cornell": ((abi.FILTER_GAUSSIAN, 1.0, 1.0, CORNELL_OFFSET), True),
    "default": ((abi.FILTER_GAUSSIAN, 0.75, 1.0, constructor_offset(0.75, 1.0)), True),
    "half": ((abi.FILTER_GAUSSIAN, 0.5, 2.0, constructor_offset(0.5, 2.0)), True),
    "one": ((abi.FILTER_GAUSSIAN, 1.0, 1.0, constructor_offset(1.0, 1.0)), False),     # zero radius exactly 1: -falloff is log(offset), not below it by 1e-6
    "box": ((abi.FILTER_BOX, 0.75, 1.0, constructor_offset(0.75, 1.0)), False),
    "offset0": ((abi.FILTER_GAUSSIAN, 1.0, 1.0, 0.0), False),
    "wide": ((abi.FILTER_GAUSSIAN, 2.0, 1.0, CORNELL_OFFSET), False),
}


def _pack_filter(name):
    g = np.load(os.path.join(GOLDEN, name + ".golden.npz"))
    f = abi.Options.from_buffer_copy(g["options"].tobytes()).filter
    return f.type, f.width, f.falloff, f.offset


def _offsets():
    out = {name: _pack_filter(name)[3] for name in ("cornell", "veach", "glass")}
    for w in (0.5, 0.75, 1.0):
        out["constructor %.2f" % w] = constructor_offset(w, 1.0)
    return out


def test_the_packs_hold_the_constructors_offset():
    assert _pack_filter("cornell") == (abi.FILTER_GAUSSIAN, 1.0, 1.0, float(CORNELL_OFFSET))
    assert _pack_filter("veach")[3] == float(CORNELL_OFFSET) and _pack_filter("glass")[3] == float(CORNELL_OFFSET)
    assert CORNELL_OFFSET == F(0.5697828531265259)


@pytest.mark.parametrize("name", sorted(_offsets()))
def test_arg_zero_is_log_offset_less_a_millionth_rounded_down(name):
    offset = _offsets()[name]
    z = abi.accumulate_arg_zero(offset)
    exact = math.log(float(offset)) - 1e-6
    assert z.dtype == np.float32 and float(z) <= exact < float(np.nextafter(z, F(np.inf)))
    # e^argZero <= offset*(1 - 1e-6), and expf is within an ulp (2^-23 relative is a loose bound on one): below offset with room to spare
    assert math.exp(float(z))*(1 + 2.0**-23) < float(offset)


@pytest.mark.parametrize("name", sorted(_offsets()))
def test_expf_at_and_below_arg_zero_never_exceeds_the_offset(name):
    offset = _offsets()[name]
    z = abi.accumulate_arg_zero(offset)
    assert z < 0
    # the 2^17 floats at and below argZero (negative floats: the next one down has the next bit pattern up)
    bits = z.view(np.uint32) + np.arange(1 << 17, dtype=np.uint32)
    assert (expf(bits.view(np.float32)) <= offset).all()
    # and random arguments down to the far corner of the widest footprint the tiled kernels take (|x| < 3, falloff 1)
    rng = np.random.default_rng(int(z.view(np.uint32)))
    a = (float(z) - rng.random(100000)*(9.0 + float(z))).astype(np.float32)
    a = np.minimum(a, z)
    assert a.min() < -8.9 and (expf(a) <= offset).all()
    # the band just above argZero is NOT claimed: there are arguments above it whose expf still exceeds the offset
    assert (expf(np.nextafter(z, F(0)) + np.arange(1, 64, dtype=F)*F(1e-6)) > offset).any()


def test_which_filters_take_the_support_form():
    L = tinsel_amd.load_library()
    for name, (f, want) in FILTERS.items():
        z = C.c_float(123.0)
        got = L.tinsel_hip_accumulate_support(int(f[0]), float(f[1]), float(f[2]), float(f[3]), C.byref(z))
        assert bool(got) == want == abi.accumulate_takes_support_form(*f), name
        if want:
            assert F(z.value) == abi.accumulate_arg_zero(f[3]) and -F(f[2]) <= F(z.value), name
    # the borderline one: the zero radius of Filter(gaussian, 1.0, 1.0) is exactly its width, 1, and the rule wants 1e-6 of margin
    f = FILTERS["one"][0]
    assert f[3] == expf(F(-1.0))[()] and -F(f[2]) > abi.accumulate_arg_zero(f[3])
    # the packs' filters all take it
    for name in ("cornell", "veach", "glass"):
        assert abi.accumulate_takes_support_form(*_pack_filter(name)), name


def test_the_tuning_has_a_full_window_value():
    assert abi.ACCUMULATE_FULL_WINDOW == 4
    assert abi.Tuning(accumulate=abi.ACCUMULATE_FULL_WINDOW).accumulate == 4


def test_the_numpy_addsample_equals_the_oracles_framebuffer():
    """tests/accumulate_reference.py on the oracle's own radiance against the oracle's own framebuffer (the reference's compiled AddSample where
    oracle/_ref is built, its C restatement otherwise)"""
    assert have_ref() or have_port()
    O = RefOracle() if have_ref() else PortOracle()
    for name in ("cornell", "veach"):
        h = O.load_pack(os.path.join(GOLDEN, name + ".pack"))
        cam, opt = O.camera_options(h)
        opt.width, opt.height = 33, 19
        acc, rad, _ = O.render_seeded(h, cam, opt, 0, 2, want_radiance=True, threads=4)
        O.free(h)
        rad4 = np.zeros((2, 19, 33, 4), np.float32)
        rad4[..., :3] = rad
        f = opt.filter
        mine = add_passes(np.zeros((19, 33, 4), np.float32), rad4, [O.pass_seed(0), O.pass_seed(1)], (f.type, f.width, f.falloff, f.offset), opt.clamp)
        assert np.array_equal(mine, acc), name

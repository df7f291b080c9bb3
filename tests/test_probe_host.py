"""The host side of the synthetic-probe tests (tests/probe_host.py), checked without a GPU: the numpy BuildCDF against the committed packs'
tables, the pack edit against the pack's own bytes, the model of ProbeSample's choice against the C restatement's ProbeSample, the C
restatement against the reference's own code where oracle/_ref is built, and the margins of tests/test_gpu_probe_synthetic.py on a model
of the alias sampler, so that what is asserted of the kernels there is known to hold for a correct sampler on the same seeds."""
import functools
import os

import numpy as np
import pytest

from tinsel_amd import abi
from tests import light_groups_reference as lg
from tests import oracle_api as oa
from tests import probe_host as ph

pytestmark = pytest.mark.skipif(not oa.have_port(), reason="oracle/libtinsel_oracle.so not built")

W, H, PASSES = ph.W, ph.H, ph.PASSES
N_MODEL = 100_000
N_ALIAS = 1_000_000          # the perturbation study's rows: those of odd and flat


# ---------------------------------------------------------------------------
# 1, 2: BuildCDF and the pack edit

@pytest.mark.parametrize("name", ["cornell_probe", "features_probe"])
def test_build_cdf_is_the_committed_tables_bit_for_bit(name):
    texels, pdf_x, cdf_x, pdf_y, cdf_y = ph.probe_sections(ph.pack(name))
    got = ph.build_cdf(texels)
    for what, a, b in zip(("pdf_x", "cdf_x", "pdf_y", "cdf_y"), got, (pdf_x, cdf_x, pdf_y, cdf_y)):
        assert a.dtype == np.float32 and np.array_equal(ph.bits(a), ph.bits(b)), (name, what)


@pytest.mark.parametrize("name", ["cornell_probe", "features_probe"])
def test_a_pack_rewritten_with_its_own_texels_is_the_same_bytes(name):
    b = ph.pack(name)
    assert ph.with_probe(b, ph.probe_sections(b)[0]) == b


def test_a_black_row_gets_the_references_nan_tables():
    p = ph.probe("blackrows")
    assert list(p.black_rows) == [0, 3, 5]
    assert np.isnan(p.pdf_x[p.black_rows]).all() and np.isnan(p.cdf_x[p.black_rows]).all() and (p.pdf_y[p.black_rows] == 0).all()
    live = np.setdiff1d(np.arange(p.H), p.black_rows)
    assert np.isfinite(p.pdf_x[live]).all() and (p.pdf_y[live] > 0).all()
    assert (p.p.reshape(p.H, p.W)[p.black_rows] == 0).all() and abs(p.p.sum() - 1.0) < 1e-12


def test_the_catalogue_is_what_it_says():
    for name in ph.LEAF_PROBES:
        p = ph.probe(name)
        assert (p.W, p.H) == ph.SIZES[name] and np.array_equal(ph.probe(name).texels, p.texels)
    odd = ph.probe("odd")
    assert (odd.p.reshape(25, 50)[:, 25] == 0).all() and 0.80 < odd.p.max() < 0.88 and int(np.argmax(odd.p)) == 9*50 + 31
    flat = ph.probe("flat")
    keep, _ = ph.vose(flat.p)
    below = np.sort(keep[keep < 1.0])
    # nearly every bin splits its draws, at thresholds spread over (0.5, 1): a scaled probability is at least 0.5 here, and so is what Vose leaves
    assert len(below) > 0.9*flat.n and below[0] < 0.55 and below[-1] > 0.95 and np.diff(below).max() < 0.05
    big = ph.probe("big")
    assert big.n == 80000 and big.n & (big.n - 1) and int(np.ceil(np.log2(big.H))) == 8 and int(np.ceil(np.log2(big.W))) == 9
    assert ph.probe("one").n == 1
    assert np.sin(np.float32(0.0/1.0)*np.float32(np.pi)) == 0.0                         # thin_9x1: v = 0 on its only row


def test_the_vectorised_generator_is_port_leaf_random():
    O = oa.PortOracle()
    seeds = np.concatenate([ph.seeds(2000), np.array([0, 1, 2**31, 2**32 - 1, 2**32 - 315645664, 3979321632], np.uint64).astype(np.uint32)])
    u1, r1, u2, r2 = ph.draws(seeds)
    for i, s in enumerate(seeds):
        r, f = O.leaf_random(int(s), 2)
        assert (u1[i], u2[i]) == (r[0], r[1]) and ph.bits(np.array([r1[i], r2[i]])).tolist() == ph.bits(f).tolist(), int(s)


# ---------------------------------------------------------------------------
# 3: the model of ProbeSample's choice against the C restatement

@pytest.mark.parametrize("name", ph.LEAF_PROBES)
def test_the_model_picks_the_texel_whose_colour_port_leaf_probe_returns(name):
    p = ph.probe(name)
    d, c, pdf, pdf2, ev = ph.port_leaf(name, N_MODEL)
    u1, r1, u2, r2 = ph.draws(ph.seeds(N_MODEL))
    want = ph.cdf_pick(p, r1, r2)
    assert (want < p.n).all() and (p.p[want] > 0).all()
    assert np.array_equal(p.texel_of(c), want)
    assert np.array_equal(ph.bits(c), ph.bits(p.texels.reshape(-1, 4)[want, :3]))
    top = want//p.W == 0                 # row 0 is the pole: sinTheta == 0 and ProbeSample returns pdf = 0 (all of thin_9x1 and of one)
    assert (pdf[top] == 0).all() and (pdf[~top] > 0).all() and np.isfinite(pdf).all()
    assert name not in ("thin_9x1", "one") or top.all()
    if len(p.black_rows):
        assert not np.isin(want//p.W, p.black_rows).any()


# ---------------------------------------------------------------------------
# 4: the C restatement against the reference's own code, on these probes

needs_ref = pytest.mark.skipif(not oa.have_ref(), reason="oracle/_ref not built")


@needs_ref
@pytest.mark.parametrize("name", ph.LEAF_PROBES)
def test_port_leaf_probe_is_ref_leaf_probe_bit_for_bit(name):
    R = oa.RefOracle()
    h = R.load_pack(ph.blob(name))
    try:
        ref = R.probe(h, ph.seeds(N_MODEL))
    finally:
        R.free(h)
    for what, a, b in zip(("dir", "color", "pdf", "pdfOfDir", "evalOfDir"), ph.port_leaf(name, N_MODEL), ref):
        same = ph.bits(a) == ph.bits(b)
        if what == "pdfOfDir":          # 0*NaN beside a black row: a NaN is a NaN, whatever its sign
            same |= np.isnan(a) & np.isnan(b)
        assert same.all(), (name, what, int((~same).sum()))


@needs_ref
@pytest.mark.parametrize("name", ph.RENDER_PROBES)
def test_port_render_is_ref_render_on_the_rewritten_pack(name):
    b = ph.blob(name)
    cam, opt = lg.frame(b, W, H)
    R = oa.RefOracle()
    h = R.load_pack(b)
    try:
        acc, rad, _ = R.render_seeded(h, cam, opt, 0, PASSES, threads=min(16, os.cpu_count() or 1), want_radiance=True)
    finally:
        R.free(h)
    pacc, prad = ph.port_render(name, radiance=True)
    assert np.array_equal(ph.bits(prad), ph.bits(rad)) and np.array_equal(ph.bits(pacc), ph.bits(acc))


# ---------------------------------------------------------------------------
# 5: the scene sees its probe

@pytest.mark.parametrize("name", ph.RENDER_PROBES)
def test_the_render_is_finite_and_depends_on_the_probe(name):
    acc, _ = ph.port_render(name)
    own, _ = ph.port_render(None)
    assert np.isfinite(acc).all() and acc[..., :3].any()
    assert np.array_equal(acc[..., 3], own[..., 3]) and not np.array_equal(acc[..., :3], own[..., :3])


def test_cornell_probe_is_blind_to_its_probe():
    """why the renders above are of features_probe: no path of cornell_probe leaves the box (tests/golden/make_golden.py)"""
    b = ph.pack("cornell_probe")
    cam, opt = lg.frame(b, W, H)
    O = oa.PortOracle()
    out = []
    for texels in (None, ph.probe("flat").texels, ph.probe("odd").texels):
        h = O.load_pack(b if texels is None else ph.with_probe(b, texels))
        out.append(O.render_seeded(h, cam, opt, 0, PASSES, threads=min(16, os.cpu_count() or 1))[0])
        O.free(h)
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[2]) and out[0][..., :3].any()


# ---------------------------------------------------------------------------
# 6: the margins of the alias checks, on a model

def caught(name, texel, factor):
    u1, r2, out = ph.model_rows(name, N_ALIAS, texel, factor)
    p = ph.probe(name).p
    try:
        lower, upper, width = ph.alias_structure(u1, r2, out, len(p))
    except ph.AliasStructureError:
        return True
    return not ph.in_brackets(p, lower, upper).all()


@pytest.mark.parametrize("name", ph.LEAF_PROBES)
def test_alias_structure_on_a_correct_table(name):
    """The model on the GPU test's own seeds and row counts (1,000,000 on odd, flat and blackrows, 200,000 on the others): everything
    test (b) of tests/test_gpu_probe_synthetic.py asserts of the kernel's texels holds for a correct table.  Measured:

        probe       total bracket width (cap)    worst texel of the frequency check (of 6 standard deviations)
        odd         0.00487  (0.01)              3.41
        flat        0.00444  (0.01)              3.78
        one         0.00000  (0.01)              0.00
        thin_7x3    0.00042  (0.01)              2.90
        thin_1x9    0.00012  (0.01)              1.54
        thin_9x1    0.00015  (0.01)              1.88
        big         0.95234  (1.48987, ph.alias_width_cap: 2.5 rows a bin)      3.70
        blackrows   0.00023  (0.01)              2.36"""
    p = ph.probe(name)
    rows = ph.alias_rows(name)
    u1, r2, out = ph.model_rows(name, rows)
    lower, upper, width = ph.alias_structure(u1, r2, out, p.n)
    print("%s: total bracket width %.5f of the mass (cap %.5f)" % (name, width, ph.alias_width_cap(name)))
    assert ph.in_brackets(p.p, lower, upper).all()
    assert width <= ph.alias_width_cap(name)
    assert (p.p[out] > 0).all()
    assert ph.frequencies_ok(p.p, out, name)


def test_alias_structure_refuses_what_is_no_alias_sampler():
    p = ph.probe("flat")
    u1, r2, out = ph.model_rows("flat", N_ALIAS)
    k = ((u1.astype(np.uint64)*np.uint64(p.n)) >> np.uint64(32)).astype(np.int64)
    # a bin that hands draws to two texels
    two = out.copy()
    row = int(np.flatnonzero(out != k)[0])
    two[row] = (out[row] + 1) % p.n if (out[row] + 1) % p.n != k[row] else (out[row] + 2) % p.n
    with pytest.raises(ph.AliasStructureError):
        ph.alias_structure(u1, r2, two, p.n)
    # a bin whose kept and given-away draws interleave: the CDF sampler's texels are no alias sampler's
    u1b, r1b, u2b, r2b = ph.draws(ph.seeds(N_ALIAS))
    with pytest.raises(ph.AliasStructureError):
        ph.alias_structure(u1b, r2b, ph.cdf_pick(p, r1b, r2b), p.n)


def test_what_alias_structure_catches_of_a_wrong_table():
    """One texel's probability scaled in the MODEL's table (never in the product), the true probabilities held to the brackets.
    Smallest factor - 1 caught, of 1, 0.3, 0.1, 0.03, 0.01, 0.003, 0.001, 0.0003, at 1,000,000 rows (measured; the test prints them again):

        flat   a texel of median probability (p = 8.7e-4)    0.001    (0.0003 passes unnoticed)
        odd    the bright texel (84 % of the mass)           0.003    (0.001 passes)
        odd    a dim texel (p = 1e-5)                        0.3      (0.1, 0.03 and 0.01 pass)

    The dim texel's bin keeps 1 % of its 800 draws, ten rows, and a texel's bracket is as wide as 1/n times the r2 spacing of the rows of
    its bin, whatever its p.  That is why `flat` is in the catalogue, and why the frequency check stands beside this one.
    Asserted is what the bracket widths promise.  A bracket is on average at most 2*(2 + aliases)/(rows per bin) of 1/n wide, under 1 %
    of a flat texel's p at 868 rows per bin: 3 % on a flat texel must be caught.  On odd's bright texel 1 % moves 0.84 % of the mass
    against a total width of 0.5 %: it must be caught."""
    flat, odd = ph.probe("flat"), ph.probe("odd")
    mid = int(np.argsort(flat.p)[flat.n//2])
    bright = int(np.argmax(odd.p))
    dim = int(np.argmin(np.abs(odd.p - 1e-5)))
    ladder = (1.0, 0.3, 0.1, 0.03, 0.01, 0.003, 0.001, 0.0003)
    for what, name, texel in (("flat, a median texel", "flat", mid), ("odd, the bright texel", "odd", bright), ("odd, a dim texel", "odd", dim)):
        hits = [f for f in ladder if caught(name, texel, 1.0 + f)]
        print("%s (p = %.3g): caught at %s" % (what, ph.probe(name).p[texel], hits))
    assert caught("flat", mid, 1.03) and caught("flat", mid, 1/1.03)
    assert caught("odd", bright, 1.01)


def test_two_cdf_renders_of_the_reference_pass_the_mean_statistic():
    """The second statistic of the GPU test's (e) on the C restatement alone: 64 x 48, 64 passes from pass 0 against 64 passes from
    pass 5000.  Measured:

        odd    L2 3.772e-01    mean of the difference image 1.95 standard errors from 0
        big    L2 1.256e-01    mean of the difference image 1.69 standard errors from 0

    (The L2 between the two is the yardstick of (e): there is nothing to hold it to here.)"""
    for name in ("odd", "big"):
        a, _ = ph.port_render(name, 64, 48, 0, 64)
        b, _ = ph.port_render(name, 64, 48, 5000, 64)
        z = ph.mean_difference_z(a, b)
        print("%s: two CDF renders on other passes: L2 %.4e, mean difference %.2f standard errors from 0" % (name, oa.image_l2(a, b), z))
        assert z <= 6.0

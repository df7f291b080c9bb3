"""The tolerance arithmetic arm's LEAF FUNCTIONS (tinsel_fast.hip's k_leaf, launched by tinsel_hip_leaf after
set_arithmetic(ARITH_FAST)) held, function by function, to a float64 statement of the same operation (tests/shade_f64.py, pinned to the
reference by tests/test_shade_f64.py).  The whole-path checks of tests/test_gpu_fast_accuracy.py call a path "on track" within 1e-3: a
pdf scaled by 1.0005 passes them.  Here every table is evaluated twice on the same rows -- the exact arm, then the tolerance arm, one
renderer per scene -- and the yardstick is never the code under test: it is the exact arm (which tests/test_gpu_leaf.py holds to the
reference's own functions) measured against the same float64 statement.

MARGINS (isect_f64.error_margins, unchanged): the tolerance arm's error distribution may be at most 4x the exact arm's at the median, the
99th and the 99.9th percentile, 16x at the maximum.  Error is relative to max(|x64|, 1e-6 max|row|) for f, pdf, PrimitiveSample's
position, expf and acosf; the angle to the statement's vector for directions and normals; absolute for sinf / cosf (components of unit
vectors) and atan2f (an angle that becomes a texture coordinate).

ROWS (tests/fast_leaf_rows.py): 65,536 per table from fixed seeds; per material the families random, grazing and near-mirror.
  * BSDFEval per channel and BSDFPdf, per material and family -- on the rows where the statement is not exactly 0 (an opaque material
    seen from below: there both arms must return exactly 0; a 0 above the surface is Fr's difference cancelling at equal indices,
    which no fp32 arithmetic reproduces: neither compared nor demanded);
  * BSDFSample direction and pdf on the rows where both arms took the statement's lobe from the statement's stream position, to the
    statement's side of the surface (`Dot(L, n) <= 0` picks BSDFPdf's formula as the lobe picks the sampler).  A row where an arm did
    not is a BRANCH ROW: counted, not compared; the tolerance arm's share may be at most 4x the exact arm's plus 1e-4 of the rows (the
    complement of test_gpu_leaf's 0.9999);
  * rows on which the statement itself is within 1e-6 of a comparison flipping (|n.L|, SinThetaT2 - 1, sin2ThetaT - 1, a draw against
    its threshold) or is not finite are excluded from the host alone: under 1 % of every table (asserted here and on the CPU);
  * PrimitiveSample position and normal; GenerateRay origin and direction at 1920 x 1080; sinf / cosf on [0, 2 pi], expf(-x) on
    [0, 80], acosf on [-1, 1] and atan2f on 1 M values; Random bit for bit; the probe (op 6, features_probe): the texel equal to the
    exact arm's on at least 1 - 4 s - 0.005 of the rows (s: tests/golden/fast_leaf_yardstick.json), direction and pdf by the margins;
  * EDGE ROWS, class only (magnitudes there are ill-conditioned in any fp32 arithmetic): n.V in {1, 1e-3, 1e-7, 0}, L = -V, n.L
    exactly 0, the critical angle for 1.5 -> 1, etaI == etaO, a denormal component.  Per output word the class -- NaN, +inf, -inf,
    finite (zero and denormal count as finite: the arm flushes) -- equals the exact arm's, and `pdf > 0`, which decides whether the
    integrator keeps a sample, holds in both or in neither.  The same on every row of the random family (there `pdf > 0` only where the
    statement's pdf is not within 1e-6 of 0), and on the 101 seeds of all 2^32 whose r1 is exactly 1.0f, where the cosine lobe's
    Max(0, .) is all that keeps z from NaN.
  * BSDFSample's pdf is compared with the statement's BSDFPdf at the direction the arm itself returned (the direction has its own
    table): what the integrator divides by, for the direction it was given.  Every table has at least 1,000 rows.
  * The tables found two defects, both repaired in the tolerance build: etaI/etaO of equal indices was 1 + 2^-23 under v_rcp_f32
    (tn_bsdf.h, index_ratio), and expf carried x log2 e in one float, 48x the exact arm's error at the 99th percentile (tn_math.h).

Every TABLE / BRANCH / EDGE line is printed before anything is asserted; measured figures: profiles/fast_arm_accuracy.md section 7."""
import json
import os

import numpy as np
import pytest

import tinsel_amd
from tinsel_amd import abi
from tests import fast_leaf_rows as flr
from tests import isect_f64 as f64
from tests import oracle_api as oa
from tests import shade_f64 as s64

pytestmark = pytest.mark.gpu

N = flr.N
EXCLUDED = 0.01
BRANCH_SLACK = 1e-4
EDGE_LISTED = 0.02
MIN_ROWS = 1000
# Edge rows that cannot have the exact arm's class, by (pack, primitive, "eval" | "sample") -> {row index: the arithmetic reason}.  At most
# 2 % of a table.
EDGE_EXCEPTIONS = {}


@pytest.fixture(scope="module")
def renderer():
    """one renderer per scene, shared by every table of the module"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = tinsel_amd.create_gpu_renderer(flr.scene(name))
        return made[name]
    yield get
    for r in made.values():
        r.close()


def _both(r, op, index, n, stride, **kw):
    """the same rows through the exact arm's k_leaf, then the tolerance arm's"""
    try:
        r.set_arithmetic(abi.ARITH_EXACT)
        exact = r.leaf(op, index, n, stride, **kw)
        r.set_arithmetic(abi.ARITH_FAST)
        fast = r.leaf(op, index, n, stride, **kw)
    finally:
        r.set_arithmetic(abi.ARITH_EXACT)
    return exact, fast


class _Tables:
    """prints every table, remembers the ones over their margin, asserts at the end"""

    def __init__(self):
        self.over = {}

    def add(self, what, e_fast, e_exact):
        e_fast, e_exact = (np.where(np.isnan(e), np.inf, e) for e in (np.asarray(e_fast, np.float64), np.asarray(e_exact, np.float64)))
        if len(e_fast) < MIN_ROWS:          # (a change of the rows or the masks that empties a table must not pass for agreement)
            print("TABLE %-44s n %6d" % (what, len(e_fast)))
            self.over[what] = "%s: %d rows, fewer than %d" % (what, len(e_fast), MIN_ROWS)
            return
        try:
            f64.error_margins(what, e_fast, e_exact)
        except AssertionError as err:
            self.over[what] = str(err)

    def check(self):
        assert not self.over, "\n".join(self.over.values())


def _classes(a):
    """per word: 0 finite (zero and denormal included), 1 NaN, 2 +inf, 3 -inf"""
    a = np.asarray(a, np.float32)
    return np.select([np.isnan(a), a == np.inf, a == -np.inf], [1, 2, 3], 0)


def _same_class(what, exact, fast, pdf_col, rows=None, sign=None, listed=()):
    """class per word and `pdf > 0` of the tolerance arm against the exact arm, on `rows` (a mask; default all), the `pdf > 0` half on
    `sign` (a mask; default `rows`) -> (the rows that differ and are not listed, the listed rows that do not differ)"""
    rows = np.ones(len(exact), bool) if rows is None else rows
    sign = rows if sign is None else sign & rows
    differ = (rows & (_classes(exact) != _classes(fast)).any(axis=1)) | (sign & ((exact[:, pdf_col] > 0) != (fast[:, pdf_col] > 0)))
    bad = [int(i) for i in np.nonzero(differ)[0] if int(i) not in listed]
    stale = [int(i) for i in listed if not differ[int(i)]]
    print("EDGE  %-44s rows %6d  class or pdf > 0 differs on %d (listed %d)" % (what, int(rows.sum()), int(differ.sum()), len(listed)))
    for i in bad[:16]:
        print("      row %d: exact %s  tolerance %s" % (i, exact[i].tolist(), fast[i].tolist()))
    return bad, stale


# ---------------------------------------------------------------------------
# BSDFEval / BSDFPdf / BSDFSample

def _took(out, s, normal):
    """did the arm whose BSDFSample records are `out` take the statement's branch?  The lobe (the BSDFType it reports), the stream position
    (the generator's two words afterwards) and -- on the lobes whose pdf is BSDFPdf's -- the side of the surface the direction it returns is
    on: `Dot(L, n) <= 0` decides which of BSDFPdf's two formulas gives the pdf, like the lobe decides the sampler"""
    same = (out[:, 5:7].view(np.uint32) == s["state"]).all(axis=1) & (out[:, 4].view(np.int32) == s["type"])
    lobed = ~np.isin(s["lobe"], (s64.LOBE_REFRACT, s64.LOBE_TIR))
    side = ((out[:, :3].astype(np.float64)*normal).sum(axis=1) <= 0) == ((s["L"]*normal).sum(axis=1) <= 0)
    return same & (side | ~lobed)


def _bsdf_tables(r, name, prim, T, notes, families=flr.FAMILIES):
    m = flr.material(name, prim)
    for family in families:
        tag = "%s %d %s" % (name, prim, family)
        rows = flr.eval_rows(family, name, prim)
        Nn, V, L, ei, eo = s64._split(rows)
        f, pdf = s64.bsdf_eval(m, ei, eo, Nn, V, L), s64.bsdf_pdf(m, ei, eo, Nn, V, L)
        out = s64.near_flip_eval(m, rows) | ~np.isfinite(f).all(axis=1) | ~np.isfinite(pdf)
        exact, fast = _both(r, 2, prim, N, 4, rows=rows)
        keep = ~out
        below = (Nn*L).sum(axis=1) <= 0             # (a 0 there is the formula's constant; one above the surface is a difference that cancelled)
        for c, ch in enumerate("rgb"):
            live = keep & (f[:, c] != 0)
            ee, ef = s64.rel_error(exact[:, :3], f)[:, c], s64.rel_error(fast[:, :3], f)[:, c]
            T.add("%s BSDFEval %s" % (tag, ch), ef[live], ee[live])
            zero = keep & below & (f[:, c] == 0)
            if not ((exact[zero, c] == 0) & (fast[zero, c] == 0)).all():
                notes.append("%s BSDFEval %s: not exactly 0 where the statement is" % (tag, ch))
        live = keep & (pdf != 0)
        T.add("%s BSDFPdf" % tag, s64.rel_error(fast[:, 3], pdf)[live], s64.rel_error(exact[:, 3], pdf)[live])
        zero = keep & below & (pdf == 0)
        if not ((exact[zero, 3] == 0) & (fast[zero, 3] == 0)).all():
            notes.append("%s BSDFPdf: not exactly 0 where the statement is" % tag)
        print("EXCL  %-44s %.5f" % (tag + " eval", out.mean()))
        if not out.mean() < EXCLUDED:
            notes.append("%s: %.4f of the eval rows excluded" % (tag, out.mean()))
        # `pdf > 0` is a comparison too, and a statement pdf within 1e-6 of 0 above the surface is within 1e-6 of it flipping: at transmission 1
        # the pdf is Lerp(brdfPdf, F pdfSpec, 1) = brdfPdf + (F pdfSpec - brdfPdf), which fp32 resolves to the last bit of brdfPdf (1e-8), and
        # between equal indices F is 0.  Such rows stay in the tables; only their `pdf > 0` is not compared (family random, below)
        sign_eval = keep & (below | (np.abs(pdf) >= s64.FLIP))

        rows8, seeds = flr.sample_rows(family, name, prim)
        s = s64.bsdf_sample(m, rows8, seeds)
        exact_s, fast_s = _both(r, 3, prim, N, 7, rows=rows8, seeds=seeds)
        host = ~s["near"]
        took = [_took(o, s, Nn) for o in (exact_s, fast_s)]
        share = [float((~t & host).sum())/max(1, int(host.sum())) for t in took]
        print("BRANCH %-43s rows %6d  another lobe, stream position or side: tolerance %.6f / exact %.6f   (near a flip, excluded: %.5f)" % (
            tag + " BSDFSample", int(host.sum()), share[1], share[0], s["near"].mean()))
        if not share[1] <= 4*share[0] + BRANCH_SLACK:
            notes.append("%s BSDFSample: branch rows %.6f of the tolerance arm against %.6f of the exact arm" % (tag, share[1], share[0]))
        if not s["near"].mean() < EXCLUDED:
            notes.append("%s: %.4f of the sample rows excluded" % (tag, s["near"].mean()))
        both = host & took[0] & took[1]
        live = both & (s["lobe"] != s64.LOBE_TIR) & np.isfinite(s["pdf"])
        T.add("%s BSDFSample dir" % tag, f64.angle(fast_s[live, :3], s["L"][live]), f64.angle(exact_s[live, :3], s["L"][live]))
        # The pdf is held to the statement of BSDFSample's last line, BSDFPdf, at the direction THE ARM RETURNED (on the refraction branch
        # it does not depend on the direction).  At the statement's own direction the pdf table would measure the direction a second time:
        # BSDFPdf takes the half vector again from L + V, and where the lobe returns L next to -V one ulp of L decides the sign of
        # L.H = (|L|^2 + L.V)/|L + V|, past which Max(1e-6, L.H) makes the pdf a hundred times larger; at the roughness floor one rounding
        # of sinThetaHalf turns that half vector by hundreds of lobe widths.  The direction table holds the direction; this one holds
        # what the integrator divides by for the direction it was given.  No row is excluded for it.
        lobed = ~np.isin(s["lobe"], (s64.LOBE_REFRACT, s64.LOBE_TIR))
        V8, ei8, eo8 = rows8[:, 3:6].astype(np.float64), rows8[:, 6].astype(np.float64), rows8[:, 7].astype(np.float64)
        own = [np.where(lobed, s64.bsdf_pdf(m, ei8, eo8, Nn, V8, o[:, :3].astype(np.float64)), s["pdf"]) for o in (exact_s, fast_s)]
        lp = live & np.isfinite(own[0]) & np.isfinite(own[1]) & (own[0] != 0) & (own[1] != 0)
        T.add("%s BSDFSample pdf" % tag, s64.rel_error(fast_s[lp, 3], own[1][lp]), s64.rel_error(exact_s[lp, 3], own[0][lp]))

        if family == "random":          # class and `pdf > 0` on every row the host does not exclude: no exceptions here
            sign_sample = (s["lobe"] == s64.LOBE_TIR) | (np.abs(s["pdf"]) >= s64.FLIP)
            for what, e_, f_, k_, g_ in (("eval", exact, fast, keep, sign_eval), ("sample", exact_s[:, :4], fast_s[:, :4], both, sign_sample)):
                bad, _ = _same_class("%s %s" % (tag, what), e_, f_, 3, rows=k_, sign=g_)
                if bad:
                    notes.append("%s %s: class or pdf > 0 differs on rows %s" % (tag, what, bad[:16]))


@pytest.mark.parametrize("name,prim", flr.MATERIALS)
def test_bsdf_tables(renderer, name, prim):
    T, notes = _Tables(), []
    _bsdf_tables(renderer(name), name, prim, T, notes)
    assert not notes, "\n".join(notes)
    T.check()


def _edge_rows():
    """hand-made rows about n = (0, 0, 1) -> (eval rows [k, 11], what each is)"""
    c_crit = float(np.sqrt(1.0 - (1.0/1.5)**2))                # n.V at the critical angle for 1.5 -> 1
    views = [("n.V=1", (0.0, 0.0, 1.0)), ("n.V=1e-3", (np.sqrt(1 - 1e-6), 0.0, 1e-3)), ("n.V=1e-7", (1.0, 0.0, 1e-7)), ("n.V=0", (1.0, 0.0, 0.0)),
             ("critical", (1.0/1.5, 0.0, c_crit)), ("denormal V", (1e-40, 0.6, 0.8))]
    rows, what = [], []
    for vn, v in views:
        v = np.array(v, np.float64)
        lights = [("L=-V", -v), ("n.L=0", np.array([0.0, 1.0, 0.0])), ("mirror", np.array([-v[0], -v[1], v[2]])),
                  ("up", np.array([0.3, 0.4, np.sqrt(0.75)])), ("down", np.array([0.3, 0.4, -np.sqrt(0.75)])), ("denormal L", np.array([-1e-40, 0.6, 0.8]))]
        for ln, l in lights:
            for eta in ((1.0, 1.5), (1.5, 1.0), (1.0, 1.0), (1.5, 1.5)):
                rows.append([0.0, 0.0, 1.0] + list(v) + list(l) + list(eta))
                what.append("%s, %s, eta %g -> %g" % (vn, ln, eta[0], eta[1]))
    return np.array(rows, np.float32), what


def _edge_sample_rows():
    """BSDFSample from the edge rows' views and index pairs, eight seeds each -> (rows [k, 8], seeds [k], what each is)"""
    rows, what = _edge_rows()
    first = np.array([w.split(", ")[1] == "L=-V" for w in what])                                    # (one row per view and index pair)
    views = np.ascontiguousarray(np.concatenate([rows[first, 0:6], rows[first, 9:11]], axis=1))
    names = [w.replace(", L=-V", "") for w, k in zip(what, first) if k]
    rows8 = np.repeat(views, 8, axis=0)
    seeds = np.random.default_rng([20261021, 4]).integers(0, 2**32, size=len(rows8), dtype=np.uint64).astype(np.uint32)
    return rows8, seeds, ["%s, seed %d" % (names[i//8], i % 8) for i in range(len(rows8))]


@pytest.mark.parametrize("name,prim", flr.MATERIALS)
def test_bsdf_edge_rows_by_class(renderer, name, prim):
    r = renderer(name)
    rows, what = _edge_rows()
    notes = []
    exact, fast = _both(r, 2, prim, len(rows), 4, rows=rows)
    rows8, seeds, what8 = _edge_sample_rows()
    exact_s, fast_s = _both(r, 3, prim, len(rows8), 7, rows=rows8, seeds=seeds)
    # (a row on which the tolerance arm took another lobe or stream position than the exact arm is a branch row: counted, its words not compared)
    same_branch = (exact_s[:, 4:7].view(np.uint32) == fast_s[:, 4:7].view(np.uint32)).all(axis=1)
    print("EDGE  %-44s rows %6d  BSDFSample on the exact arm's lobe and stream position: %d" % ("%s %d" % (name, prim), len(rows8), int(same_branch.sum())))
    if not (~same_branch).sum() <= EDGE_LISTED*len(rows8):
        notes.append("%s %d sample: another lobe or stream position than the exact arm on rows %s" % (name, prim, np.nonzero(~same_branch)[0].tolist()))
    for table, e_, f_, k_, w_ in (("eval", exact, fast, None, what), ("sample", exact_s[:, :4], fast_s[:, :4], same_branch, what8)):
        listed = EDGE_EXCEPTIONS.get((name, prim, table), {})
        assert len(listed) <= EDGE_LISTED*len(e_), "more than 2 % of the table listed"
        bad, stale = _same_class("%s %d %s" % (name, prim, table), e_, f_, 3, rows=k_, listed=listed)
        for i in bad[:16]:
            print("      row %d is %s" % (i, w_[i]))
        if bad:
            notes.append("%s %d %s: class or pdf > 0 differs on rows %s" % (name, prim, table, bad))
        if stale:
            notes.append("%s %d %s: rows %s are listed but agree" % (name, prim, table, stale))
    assert not notes, "\n".join(notes)


def test_the_cosine_lobe_where_r1_is_one(renderer):
    """CosineSampleHemisphere at r1 == 1.0f (fast_leaf_rows.R1_ONE_SEEDS): z = sqrt(Max(0, 1 - cos^2 - sin^2)) of a difference that is a
    rounding error of either sign -- without the Max, z and with it the direction and the pdf are NaN on about half of these rows.  Class
    only: z is 0 or a few 1e-4 by the last bit of the difference; every word finite in both arms, `pdf > 0` in both or in neither where
    the statement's direction is not within 1e-6 of the surface (on the cosine lobe it is IN it: z = 0 in float64)"""
    name, prim = "features", 0
    r, m = renderer(name), flr.material(name, prim)
    rows, seeds = flr.r1_one_rows()
    s = s64.bsdf_sample(m, rows, seeds)
    cosine = s["lobe"] == s64.LOBE_COSINE
    exact, fast = _both(r, 3, prim, len(rows), 7, rows=rows, seeds=seeds)
    for o in (exact, fast):                                     # (transmission 0, subsurface 0: no draw is compared with a computed value)
        assert np.array_equal(o[:, 5:7].view(np.uint32), s["state"]) and np.array_equal(o[:, 4].view(np.int32), s["type"])
    print("EDGE  %-44s rows %6d  on the cosine lobe %d; z of the exact arm 0 on %d, of the tolerance arm on %d" % (
        "r1 == 1", len(rows), int(cosine.sum()), int(((exact[:, :3]*rows[:, :3]).sum(axis=1)[cosine] == 0).sum()),
        int(((fast[:, :3]*rows[:, :3]).sum(axis=1)[cosine] == 0).sum())))
    assert cosine.sum() >= len(rows)//4
    assert np.isfinite(exact[:, :4]).all() and np.isfinite(fast[:, :4]).all()
    bad, _ = _same_class("r1 == 1 sample", exact[:, :4], fast[:, :4], 3, sign=~s["near"])
    assert not bad, bad


# ---------------------------------------------------------------------------
# PrimitiveSample, GenerateRay, Random, libm, probe

@pytest.mark.parametrize("name,prim", flr.LIGHTS)
def test_primitive_sample_tables(renderer, name, prim):
    r, T = renderer(name), _Tables()
    S = f64.Statement(flr.scene(name))
    times, seeds = flr.light_rows(name, prim)
    s = s64.primitive_sample(S, prim, times[:, 0], seeds)
    exact, fast = _both(r, 5, prim, N, 8, rows=times, seeds=seeds)
    for o in (exact, fast):                                     # the draws and the triangle chosen: integer and float32 comparisons
        assert np.array_equal(o[:, 6:8].view(np.uint32), s["state"])
    tag = "%s %d %s PrimitiveSample" % (name, prim, S.kind(prim))
    T.add(tag + " pos", s64.rel_error(fast[:, :3], s["pos"]).max(axis=1), s64.rel_error(exact[:, :3], s["pos"]).max(axis=1))
    T.add(tag + " normal", f64.angle(fast[:, 3:6], s["normal"]), f64.angle(exact[:, 3:6], s["normal"]))
    T.check()


def test_generate_ray_table(renderer):
    r, T = renderer("features"), _Tables()
    cam = flr.scene("features").camera
    xy = flr.camera_rows()
    o, d = s64.generate_ray(cam, 1920, 1080, xy)
    exact, fast = _both(r, 1, 0, N, 6, rows=xy, camera=cam, width=1920, height=1080)
    T.add("GenerateRay origin", s64.rel_error(fast[:, :3], o).max(axis=1), s64.rel_error(exact[:, :3], o).max(axis=1))
    T.add("GenerateRay dir", f64.angle(fast[:, 3:6], d), f64.angle(exact[:, 3:6], d))
    T.check()


def test_random_is_bit_exact_in_the_tolerance_arm(renderer):
    """the integer generator must not feel the flags"""
    r = renderer("features")
    seeds = np.random.default_rng([20261021, 0]).integers(0, 2**32, size=N, dtype=np.uint64).astype(np.uint32)
    seeds[:4] = [0, 1, 0xffffffff, 0x80000000]
    exact, fast = _both(r, 0, 0, N, 8, seeds=seeds)
    assert np.array_equal(exact.view(np.uint32), fast.view(np.uint32))
    g = s64.Random(seeds)
    for k in range(4):
        word = g.rand()
        assert np.array_equal(fast[:, k].view(np.uint32), word)
        assert np.array_equal(fast[:, 4 + k].astype(np.float64), word.astype(np.float32).astype(np.float64)*2.0**-32)


def _libm_tables(r, T):
    rng = np.random.default_rng([20261021, 7])
    n = 1 << 20
    x = np.concatenate([rng.random(n//2)*2*np.pi, rng.random(n//2)*80.0]).astype(np.float32)
    y = (rng.random(n)*2 - 1).astype(np.float32)
    x[:4], y[:4] = [0.0, np.float32(np.pi/2), np.float32(np.pi), np.float32(2*np.pi)], [1.0, -1.0, 0.0, 0.5]
    exact, fast = _both(r, 7, 0, n, 5, rows=np.stack([x, y], axis=1))
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    ang = slice(0, n//2)
    T.add("sinf [0, 2 pi] (absolute)", np.abs(fast[ang, 0] - np.sin(x64[ang])), np.abs(exact[ang, 0] - np.sin(x64[ang])))
    T.add("cosf [0, 2 pi] (absolute)", np.abs(fast[ang, 1] - np.cos(x64[ang])), np.abs(exact[ang, 1] - np.cos(x64[ang])))
    ex = np.exp(-x64)
    T.add("expf(-x) [0, 80]", s64.rel_error(fast[:, 2], ex), s64.rel_error(exact[:, 2], ex))
    ac = np.arccos(y64)
    T.add("acosf [-1, 1]", s64.rel_error(fast[:, 3], ac), s64.rel_error(exact[:, 3], ac))
    at = np.arctan2(y64, (x - np.float32(3.0)).astype(np.float64))                     # (op 7 subtracts in float32: that difference is the input)
    T.add("atan2f(y, x - 3) (absolute)", np.abs(fast[:, 4] - at), np.abs(exact[:, 4] - at))


def test_libm_tables(renderer):
    T = _Tables()
    _libm_tables(renderer("features"), T)
    T.check()


def test_expf_at_its_ends(renderer):
    """expf where the [0, 80] table never goes (op 8's third word is expf(y)): NaN, the infinities, the arguments at which the tolerance
    build clamps (-104: below the smallest denormal; 89: above FLT_MAX) and the neighbours of underflow and overflow.  Class and value:
    NaN stays NaN, -inf and everything from -104 down give 0, exp(-103) is the smallest denormal or flushed, +inf and everything from
    88.73 up give +inf, in both arms"""
    r = renderer("features")
    y = np.array([np.nan, -np.inf, np.inf, -104.0, 89.0, -1e30, 1e30, -87.0, 88.0, 88.73, -103.0, 0.0, -0.0], np.float32)
    rows = np.stack([np.ones_like(y), y], axis=1)
    exact, fast = _both(r, 8, 0, len(y), 4, rows=rows)
    print("EDGE  expf(y): y %s\n      exact %s\n      tolerance %s" % (y.tolist(), exact[:, 2].tolist(), fast[:, 2].tolist()))
    assert np.array_equal(_classes(exact[:, 2]), _classes(fast[:, 2]))
    for o in (exact, fast):
        assert np.isnan(o[0, 2]) and (o[[1, 3, 5], 2] == 0).all() and 0 <= o[10, 2] <= 2.0**-149 and np.isinf(o[[2, 4, 6, 9], 2]).all() and (o[[11, 12], 2] == 1).all()
    fin = [7, 8]
    ref = np.exp(y[fin].astype(np.float64))
    assert (np.abs(fast[fin, 2] - ref) <= 4*np.maximum(np.abs(exact[fin, 2] - ref), 2.0**-24*ref)).all()


def test_probe_table(renderer):
    with open(os.path.join(oa.GOLDEN, "fast_leaf_yardstick.json")) as fh:
        share = json.load(fh)["texel_differs_share"]
    r, T = renderer("features_probe"), _Tables()
    seeds = flr.probe_seeds()
    exact, fast = _both(r, 6, 0, N, 11, seeds=seeds)
    s = s64.probe_sample(flr.scene("features_probe"), seeds)
    same = (exact[:, 3:6] == fast[:, 3:6]).all(axis=1)
    print("PROBE texel equal to the exact arm's on %.6f of %d rows (the reference's two builds differ on %.6f)" % (same.mean(), N, share))
    assert same.mean() >= 1 - 4*share - 0.005
    # float64 from the exact arm's texel: the statement's searches are exact comparisons, so its texel must BE the exact arm's
    assert np.array_equal(s["color"], exact[:, 3:6])
    live = same & (s["pdf"] > 0)
    T.add("ProbeSample dir", f64.angle(fast[same, :3], s["dir"][same]), f64.angle(exact[same, :3], s["dir"][same]))
    T.add("ProbeSample pdf", s64.rel_error(fast[live, 6], s["pdf"][live]), s64.rel_error(exact[live, 6], s["pdf"][live]))
    T.check()

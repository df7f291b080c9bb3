"""tests/shade_f64.py -- the float64 statement the tolerance arm's leaf tables lean on -- pinned to the reference's own functions
(oracle/_ref's IEEE build, RefOracle() leaf entry points) on the rows of tests/test_gpu_fast_leaf.py, and to closed forms at hand-made
rows.  No GPU.

  * BSDFSample takes the reference's lobe (its BSDFType) from the reference's stream position on at least 0.9999 of the rows --
    tests/test_gpu_leaf.py's own figure for a `rand < F` comparison flipping on a last-bit F;
  * on those rows the median relative difference of f, pdf and the sampled direction (its angle) is at most 40 x 2^-24: the longest
    chain in BSDFEval is about forty rounded fp32 operations.  That median is over all the rows (test_the_median_over_all_rows).  A
    single table cannot always meet it, and not because of the statement: GTR2 / GTR1 compute t = 1 + (a^2 - 1) NDotH^2, and next to
    NDotH = 1 t is about a^2 + angle^2 while the float32 rounding of NDotH^2 is 6e-8: an error of 6e-8 / t in t, twice that in GTR2 --
    1e-5 for the clearcoat alpha 0.06 of features 0, 1e-1 at the roughness floor 0.001 -- and BSDFSample's GGX lobe puts every
    direction it returns there.  That is the reference's own float32 error.  So each table is held to forty roundings' worth instead:
    40 x max(2^-24 k, c), with c the statement's own median response to ONE float32 rounding of its inputs (every direction component
    times 1 +- 2^-24) and k the cancellation of the closing Lerps (the largest term they add and subtract over the result: a specular
    pdf of 1e-6 under a diffuse one of 0.1 at transmission 1) -- from the statement and the number format alone;
  * the rows the tables exclude from the host alone (the statement within 1e-6 of a comparison flipping, or not finite) are under 1 %
    of every table.
"""
import functools

import numpy as np
import pytest

from tests import fast_leaf_rows as flr
from tests import isect_f64 as f64
from tests import oracle_api as oa
from tests import shade_f64 as s64

needs_ref = pytest.mark.skipif(not oa.have_ref(), reason="oracle/_ref not built")

MEDIAN = 40*2.0**-24
AGREE = 0.9999
EXCLUDED = 0.01


def _ref_material(R, name, prim):
    h = R.load_pack(flr._pack(name))
    mat = R.primitive(h, prim).material
    return h, mat


def test_the_materials_hold_every_class():
    have = {}
    for name, prim in flr.MATERIALS:
        for c in flr.material(name, prim).classes():
            have.setdefault(c, []).append((name, prim))
    for c in flr.CLASSES:
        print("%-22s %s" % (c, have.get(c)))
    assert all(c in have for c in flr.CLASSES), [c for c in flr.CLASSES if c not in have]


def _perturbed(rows, rng):
    """the rows with every direction component moved by one float32 rounding (a factor 1 +- 2^-24), as float64: what the FIRST rounded
    operation of any float32 evaluation does to its inputs"""
    r = np.array(rows, np.float64)
    r[:, :-2] *= 1.0 + 2.0**-24*rng.choice([-1.0, 1.0], size=r[:, :-2].shape)
    return r


@functools.lru_cache(maxsize=None)
def _table(name, prim, family):
    """one material and family: the reference against the statement -> dict of
      e      {quantity: per-row difference} of f, pdf (BSDFEval / BSDFPdf rows), dir, sample pdf (BSDFSample rows on the reference's lobe)
      cond   {quantity: median response of the statement to one rounding of its inputs}: how many roundings' worth of difference ONE
             rounding makes on these rows -- 2^-24 where the functions are well conditioned, 1/(a^2 + angle^2) times that for GTR2 at its peak
      amp    {quantity: median of (largest term the closing Lerps add and subtract) / |result|}: the digits a float32 Lerp loses to
             cancellation; for dir, of sinThetaHalf = sqrt(1 - cosThetaHalf^2) on a GGX lobe (shade_f64.bsdf_sample's dir_terms)
      excluded, same, near   shares;   lobes   the statement's lobe counts"""
    R = oa.RefOracle()
    h, mat = _ref_material(R, name, prim)
    m = flr.material(name, prim)
    rng = np.random.default_rng(1)
    rows = flr.eval_rows(family, name, prim)
    ev = lambda r: s64.bsdf_eval(m, r[:, 9], r[:, 10], r[:, 0:3], r[:, 3:6], r[:, 6:9], terms=True) + \
        s64.bsdf_pdf(m, r[:, 9], r[:, 10], r[:, 0:3], r[:, 3:6], r[:, 6:9], terms=True)
    f_ref, pdf_ref = R.bsdf_eval(mat, rows)
    f, f_terms, pdf, pdf_terms = ev(np.asarray(rows, np.float64))
    f2, _, pdf2, _ = ev(_perturbed(rows, rng))
    out = s64.near_flip_eval(m, rows) | ~np.isfinite(f).all(axis=1) | ~np.isfinite(pdf)
    keep = ~out & np.isfinite(f_ref).all(axis=1) & np.isfinite(pdf_ref)
    # (rows on which the statement is exactly 0 -- an opaque material seen from below -- say nothing about rounding: left out of a median)
    kf, kp = keep & (f != 0).any(axis=1), keep & (pdf != 0)
    e = {"f": s64.rel_error(f_ref, f).max(axis=1)[kf], "pdf": s64.rel_error(pdf_ref, pdf)[kp]}
    cond = {"f": s64.rel_error(f2, f).max(axis=1)[kf], "pdf": s64.rel_error(pdf2, pdf)[kp]}
    with np.errstate(all="ignore"):
        amp = {"f": (f_terms/np.abs(f)).max(axis=1)[kf], "pdf": (pdf_terms/np.abs(pdf))[kp]}

    rows8, seeds = flr.sample_rows(family, name, prim)
    Lr, pr, tr, st = R.bsdf_sample(mat, rows8, seeds)
    R.free(h)
    s = s64.bsdf_sample(m, rows8, seeds)
    s2 = s64.bsdf_sample(m, _perturbed(rows8, rng), seeds)
    same = ((s["state"] == st).all(axis=1) & (s["type"] == tr))
    # (a total internal reflection leaves L and the type as the caller set them: the reference's harness and the statement both 0)
    live = same & (s["lobe"] != s64.LOBE_TIR) & np.isfinite(s["pdf"]) & (s["pdf"] > 0) & np.isfinite(pr)
    e["dir"], e["sample pdf"] = f64.angle(Lr[live], s["L"][live]), s64.rel_error(pr[live], s["pdf"][live])
    live2 = live & (s2["lobe"] == s["lobe"])
    cond["dir"], cond["sample pdf"] = f64.angle(s2["L"][live2], s["L"][live2]), s64.rel_error(s2["pdf"][live2], s["pdf"][live2])
    with np.errstate(all="ignore"):
        amp["dir"], amp["sample pdf"] = s["dir_terms"][live], (s["pdf_terms"]/s["pdf"])[live]
    draws = {s64.LOBE_FRESNEL_GGX: 4, s64.LOBE_REFRACT: 2, s64.LOBE_TIR: 2, s64.LOBE_INSIDE: 7, s64.LOBE_COSINE: 5, s64.LOBE_GGX: 4}
    assert all((s["draws"][s["lobe"] == k] == v).all() for k, v in draws.items())
    med = lambda d: {k: (float(np.median(v)) if len(v) else 0.0) for k, v in d.items()}
    # (rows on which the statement itself is within 1e-6 of a comparison flipping are no one's: the lobe is compared on the others)
    return dict(e=e, med=med(e), cond=med(cond), amp=med(amp), excluded=out.mean(), kept=keep.mean(), same=same[~s["near"]].mean(), near=s["near"].mean(),
                lobes=np.bincount(s["lobe"], minlength=6).tolist())


@needs_ref
@pytest.mark.parametrize("name,prim", flr.MATERIALS)
def test_the_statement_is_the_references_bsdf(name, prim):
    for family in flr.FAMILIES:
        t = _table(name, prim, family)
        med, cond, amp = t["med"], t["cond"], t["amp"]
        print("%-8s %2d %-11s excluded %.5f  same lobe and stream %.6f (near a flip %.5f)  median / one rounding's response / cancellation: " % (
            name, prim, family, t["excluded"], t["same"], t["near"]) + "  ".join("%s %.2e / %.2e / %.1f" % (k, med[k], cond[k], amp[k]) for k in med) +
            "  lobes %s" % t["lobes"])
        assert t["excluded"] < EXCLUDED and t["kept"] > 1 - EXCLUDED, family
        assert t["same"] >= AGREE, (family, t["same"])
        assert t["near"] < EXCLUDED, (family, t["near"])
        for k in med:
            assert med[k] <= 40*max(2.0**-24*amp[k], cond[k]), (family, k, med[k], cond[k], amp[k])
            if max(amp[k], cond[k]*2.0**24) <= 2.0:         # a table its own conditioning leaves alone meets the issue's figure by itself
                assert med[k] <= MEDIAN, (family, k, med[k])


@needs_ref
def test_the_median_over_all_rows():
    """the issue's figure: over the rows of every material and family, on the reference's lobe and stream position, the median relative
    difference of f, pdf and direction is at most 40 x 2^-24"""
    for k in ("f", "pdf", "dir", "sample pdf"):
        e = np.concatenate([_table(name, prim, family)["e"][k] for name, prim in flr.MATERIALS for family in flr.FAMILIES])
        print("%-10s rows %8d  median %.3e  (bound %.3e)" % (k, len(e), np.median(e), MEDIAN))
        assert np.median(e) <= MEDIAN, k


@needs_ref
@pytest.mark.parametrize("name,prim", flr.LIGHTS)
def test_the_statement_is_the_references_primitive_sample(name, prim):
    R = oa.RefOracle()
    h = R.load_pack(flr._pack(name))
    S = f64.Statement(flr.scene(name))
    times, seeds = flr.light_rows(name, prim)
    pos, nrm, st = R.primitive_sample(h, prim, times[:, 0], seeds)
    s = s64.primitive_sample(S, prim, times[:, 0], seeds)
    R.free(h)
    assert np.array_equal(s["state"], st)                       # (the triangle and the draws are integer and float32 comparisons: no rounding)
    ep, en = np.median(s64.rel_error(pos, s["pos"]).max(axis=1)), np.median(f64.angle(nrm, s["normal"]))
    print("%-8s %2d %-6s PrimitiveSample median pos %.2e normal %.2e" % (name, prim, S.kind(prim), ep, en))
    # a sphere's normal is Normalize(pos - p): the difference of two points rounded at their own size -- (|p| + r)/r roundings' worth
    c = 1.0
    if S.kind(prim) == "sphere":
        pp, _, sc = S.pose(prim, times[:, 0])
        c = float(np.median((np.linalg.norm(pp, axis=1) + S.prims[prim].radius*sc)/(S.prims[prim].radius*sc)))
    assert ep <= MEDIAN and en <= MEDIAN*c, (ep, en, c)


@needs_ref
def test_the_statement_is_the_references_camera_ray():
    R = oa.RefOracle()
    sc = flr.scene("features")
    xy = flr.camera_rows()
    ref = R.camera_rays(sc.camera, 1920, 1080, xy)
    o, d = s64.generate_ray(sc.camera, 1920, 1080, xy)
    assert np.array_equal(o.astype(np.float32), ref[:, :3])
    e = np.median(f64.angle(ref[:, 3:6], d))
    print("GenerateRay median angle %.2e" % e)
    assert e <= MEDIAN


@needs_ref
def test_the_statement_is_the_references_probe_sample():
    R = oa.RefOracle()
    sc = flr.scene("features_probe")
    h = R.load_pack(flr._pack("features_probe"))
    seeds = flr.probe_seeds()
    d, c, pdf, _, _ = R.probe(h, seeds)
    R.free(h)
    s = s64.probe_sample(sc, seeds)
    assert s["inside"].all()
    assert np.array_equal(s["color"], c)                        # the same texel on every row: the searches are exact comparisons
    live = pdf > 0
    ed, ep = np.median(f64.angle(d, s["dir"])), np.median(s64.rel_error(pdf[live], s["pdf"][live]))
    print("ProbeSample median dir %.2e pdf %.2e" % (ed, ep))
    assert ed <= MEDIAN and ep <= MEDIAN


def test_the_seeds_whose_second_draw_is_one():
    """fast_leaf_rows.R1_ONE_SEEDS: the second Randf() is exactly 1.0, and on an opaque material without subsurface about half of them
    take the cosine lobe, where r = sqrt(r1) = 1"""
    seeds = np.array(flr.R1_ONE_SEEDS, np.uint32)
    g = s64.Random(seeds)
    g.randf()
    assert (g.randf() == 1.0).all() and len(set(flr.R1_ONE_SEEDS)) == len(seeds) >= 64
    rows, seeds = flr.r1_one_rows()
    s = s64.bsdf_sample(flr.material("features", 0), rows, seeds)
    cosine = s["lobe"] == s64.LOBE_COSINE
    assert cosine.sum() >= len(rows)//4 and np.isfinite(s["L"]).all() and np.isfinite(s["pdf"]).all()
    assert np.abs((s["L"][cosine]*rows[cosine, 0:3].astype(np.float64)).sum(axis=1)).max() < 1e-7          # (the direction lies IN the surface)


def test_the_leaves_at_hand_made_rows():
    """closed forms: nothing here needs the reference"""
    import ctypes as C
    from tinsel_amd import abi
    one = lambda v: np.array([v], np.float64)
    # a pure diffuse material at normal incidence: f = colour/pi (every Schlick weight is 0), pdf = 0.5 cos/pi + 0.5 pdfSpec with
    # pdfSpec = 0.25 GTR2(1, 1) / 1 = 0.25/pi
    raw = abi.Material()
    C.memset(C.byref(raw), 0, C.sizeof(raw))
    raw.color.x, raw.color.y, raw.color.z = 0.5, 0.25, 0.125
    raw.roughness, raw.clearcoat_gloss = 1.0, 1.0
    m = s64.Material64(raw)
    up = np.array([[0.0, 0.0, 1.0]])
    f = s64.bsdf_eval(m, one(1.0), one(1.0), up, up, up)
    assert np.allclose(f, [[0.5/np.pi, 0.25/np.pi, 0.125/np.pi]], rtol=1e-15, atol=0)       # (specular 0: Cspec0 = 0, and FH = 0 at L.H = 1)
    assert s64.bsdf_pdf(m, one(1.0), one(1.0), up, up, up)[0] == pytest.approx(0.5/np.pi + 0.5*0.25/np.pi, rel=1e-15)
    # Fr at normal incidence for 1 -> 1.5: ((1.5 - 1)/(1.5 + 1))^2 = 0.04
    assert s64.fr(one(1.0), one(1.0), one(1.5))[0][0] == pytest.approx(0.04, rel=1e-15)
    assert s64.fr(one(1.0), one(1.5), one(1.0))[0][0] == pytest.approx(0.04, rel=1e-15)
    # Refract at the critical angle for 1.5 -> 1 (sin = 1/1.5): just inside, the transmitted ray lies in the surface; just outside, none
    n = np.array([[0.0, 0.0, 1.0]])
    for sin_i, expect in ((1/1.5 - 1e-9, True), (1/1.5 + 1e-9, False)):
        wi = np.array([[sin_i, 0.0, np.sqrt(1 - sin_i**2)]])
        ok, wt, s2 = s64.refract(wi, n, one(1.5))
        assert bool(ok[0]) is expect and abs(s2[0] - 1.0) < 1e-8
        if expect:
            assert wt[0, 0] == pytest.approx(-1.0, abs=1e-8) and abs(wt[0, 2]) < 1e-4 and np.linalg.norm(wt[0]) == pytest.approx(1.0, abs=1e-12)
    ok, wt, _ = s64.refract(n, n, one(1/1.5))                   # straight down: straight through
    assert ok[0] and np.allclose(wt, -n, atol=1e-15)
    # the GTR2 peak 1/(pi a^2) at NDotH = 1; GTR1 integrates the same way: (a^2 - 1)/(pi ln(a^2)) a^-2 at its peak
    for a in (0.001, 0.05, 0.5):
        assert s64.gtr2(one(1.0), a)[0] == pytest.approx(1.0/(np.pi*a*a), rel=1e-9)     # (1 + (a^2 - 1) cancels to 1e-16/a^2 in float64 too)
        assert s64.gtr1(one(1.0), a)[0] == pytest.approx((a*a - 1)/(np.pi*np.log(a*a)*a*a), rel=1e-9)
    # Smith at normal incidence is 1/2, Schlick at 0 and 1
    assert s64.smith_ggx(one(1.0), 0.3)[0] == pytest.approx(0.5, rel=1e-15)
    assert s64.schlick_fresnel(one(1.0))[0] == 0.0 and s64.schlick_fresnel(one(0.0))[0] == 1.0
    # the generator: Random(0)'s first draws, by the integer recurrence worked by hand (maths.h:1042-1051)
    g = s64.Random(np.array([0], np.uint32))
    s1, s2 = 315645664, 315645664 ^ 0x13ab45fe
    n1 = ((s2 ^ (((s1 << 5) | (s1 >> 27)) & 0xffffffff)) ^ ((s1*s2) & 0xffffffff)) & 0xffffffff
    assert int(g.rand()[0]) == n1
    # the samplers: unit vectors; the cosine lobe's density is z/pi, the mean of z over uniform (u1, u2) is 2/3
    u1, u2 = np.random.default_rng(1).random(100000), np.random.default_rng(2).random(100000)
    for v in (s64.uniform_sample_sphere(u1, u2), s64.uniform_sample_hemisphere(u1, u2), s64.cosine_sample_hemisphere(u1, u2), s64.ggx_half_vector(0.3, u1, u2)):
        assert np.allclose(np.linalg.norm(v, axis=1), 1.0, atol=1e-12)
    assert s64.cosine_sample_hemisphere(u1, u2)[:, 2].mean() == pytest.approx(2/3, abs=5e-3)

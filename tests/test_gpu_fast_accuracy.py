"""The tolerance arithmetic arm (tinsel_hip_set_arithmetic(TINSEL_ARITH_FAST), tinsel_fast.hip) held to per-ray and per-path checks.

A bit contract is impossible for this arm (FMA contraction, v_rcp / v_rsq / v_sqrt, fminf / fmaxf in the slab tests, denormals flushed),
so it has a tolerance contract, against a float64 statement of the same operations (tests/isect_f64.py, pinned to the reference by
tests/test_isect_f64.py) and against the exact arm -- which IS the reference's arithmetic -- on the same rays, paths and frames.

RAY QUERIES (trace_rays).  Rays per scene: the sets of tests/test_gpu_ray_query._rays drawn from the statement instead of the oracle
(65,536 random, 4,096 axis-aligned, 4,096 starting on a surface) and 1,024 more axis-aligned ones whose zeroed component is instead
-0.0, 1e-40 (a denormal this build flushes), -1e-40 or 1e-30: the slab test's 0 * inf products.
  a. at least 85 % of a scene's hit rays that do not start on a surface are CLEAR (isect_f64.clear), from host data alone; on scenes with
     a mesh above 2,000 triangles (no float64 brute force) a ray that hits that mesh is clear by the exact arm's record instead;
  b. on every clear ray the arm reports the statement's primitive; "occluded" is t64 < tmax for every clear ray and every clean miss
     whose tmax is more than 1e-4 relative from t64 -- tmax = 0.5 t, 1.5 t and inf -- no cap;
  c. the error of t and the angle of the normal against float64, on clear rays: the tolerance arm's distribution against the exact arm's
     at the median, the 99th and 99.9th percentiles (at most 4x: every operation this build swaps in has at most twice the rounding
     error of the one it replaces, and a bound against an observed percentile gets another factor 2) and at the maximum (16x);
     isect_f64.error_margins, per scene and per primitive type.  On a mesh above 2,000 triangles there is no t64: |t_fast - t_exact| <= LARGE_MESH_T t_exact;
  d. rays that start on a surface may name another primitive than the statement on at most 1 % of the scene's hit rays, and then one the
     statement places within 1e-4 max(1, |o|) of the origin, reported at such a t (isect_f64.near_tie): a near-tie, not a lost hit;
  e. b (five scenes) and c (two) again under the five pipelines and the four tuning arms of test_same_bytes_under_every_configuration,
     8,191 rays each; how many records equal the default configuration's bit for bit is printed, nothing is asserted on it.  A ray
     query runs k_query / k_query_refill whatever the pipeline, so the pipelines add no kernel here (every record is bit-equal); the
     tuning arms change where the scene lives and which walk k_query takes.
RADIANCE QUERIES, per path and by depth; FEATURE PLANES and GATHERS: see the sections below.  The tolerance build's k_walk, k_walk_rays,
k_swalk, k_step, k_shade* and k_mega are held by test_paths_under_every_pipeline alone (depth 2, three scenes).  The build's leaf
functions -- BSDF, samplers, camera ray, light sample, probe, transcendentals -- have their own tables, function by function against a
float64 statement: tests/test_gpu_fast_leaf.py.

Measured figures: profiles/fast_arm_accuracy.md."""
import functools
import json
import os
import types

import numpy as np
import pytest

import tinsel_amd
from tinsel_amd import abi
from tests import isect_f64 as f64
from tests import oracle_api as oa
from tests import test_gpu_ray_query as trq
from tests.test_gpu_ray_query import N_AXIS, N_RANDOM, N_SURFACE, _pack

gpu = pytest.mark.gpu

SCENES = ["cornell", "veach", "features", "motionblur", "many_spheres", "ajax_standin_96"] + ["fuzz:%02d" % k for k in range(8)] + \
         ["mesh:instances:1", "mesh:beyond_flat:1"]
CONFIG_SCENES = ["cornell", "glass", "ajax_standin_96", "many_spheres", "mesh:beyond_flat:1"]
ALL_SCENES = SCENES + ["glass"]
N_EDGE = 1024
EDGE_VALUES = (np.float32(-0.0), np.float32(1e-40), np.float32(-1e-40), np.float32(1e-30))
CAP = 0.01
# 2c on a mesh above 2,000 triangles: 4 x the largest |t_fast - t64|/t64 measured on the triangles of the scenes whose meshes the
# statement covers (profiles/fast_arm_accuracy.md: 1.19e-5, fuzz:02)
LARGE_MESH_T = 4*1.19e-5
PIPELINES = {"wavefront": abi.PIPELINE_WAVEFRONT, "megakernel": abi.PIPELINE_MEGAKERNEL, "split": abi.PIPELINE_WAVEFRONT_SPLIT,
             "auto": abi.PIPELINE_AUTO, "paired": abi.PIPELINE_WAVEFRONT_PAIRED}
TUNINGS = {"flat_scan=0": dict(flat_scan=0), "walk=0": dict(walk=0), "walk_min_tris=0,small_mesh_bytes=0": dict(walk_min_tris=0, small_mesh_bytes=0),
           "lds_scene=0": dict(lds_scene=0)}


class _StatementAsOracle:
    """what test_gpu_ray_query._rays asks of an oracle, answered by the float64 statement (a mesh above 2,000 triangles never hits)"""

    def __init__(self, S):
        self.S = S

    def num_primitives(self, h):
        return self.S.num_primitives

    def primitive(self, h, p):
        return types.SimpleNamespace(type=self.S.prims[p].type)

    def primitive_bounds(self, h, p):
        if self.S.boxes[p] is not None:
            return self.S.boxes[p]
        q = self.S.prims[p]                                # (a scene of one primitive has no leaf box: its ball at the shutter's ends)
        r = q.radius if q.type == abi.GEOM_SPHERE else (np.linalg.norm(q.ball[0]) + q.ball[1] if q.type == abi.GEOM_MESH else 1.0)
        lo = np.minimum(q.start[0] - r*q.start[2], q.end[0] - r*q.end[2])
        return lo, np.maximum(q.start[0] + r*q.start[2], q.end[0] + r*q.end[2])

    def primitive_intersect(self, h, p, rows):
        n = len(rows)
        if not self.S.brute(p):
            return np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros((n, 3), np.float32)
        rays = np.zeros((n, 8), np.float32)
        rays[:, 0:3], rays[:, 4:7], rays[:, 3] = rows[:, 0:3], rows[:, 3:6], rows[:, 6]
        r = self.S.intersect(p, rays)
        return np.isfinite(r["t"]).astype(np.int32), np.where(np.isfinite(r["t"]), r["t"], 0.0).astype(np.float32), r["normal"].astype(np.float32)


@functools.lru_cache(maxsize=None)
def _host(name):
    """a scene's rays and what the statement says of them: computed once on the host, shared, left unchanged"""
    scene = tinsel_amd.Scene(_pack(name))
    S = f64.Statement(scene)
    rays = trq._rays(_StatementAsOracle(S), None, 20261020 + ALL_SCENES.index(name))
    edge = rays[N_RANDOM:N_RANDOM + N_EDGE].copy()
    d = edge[:, 4:7]
    assert ((d == 0).sum(axis=1) >= 1).all()
    d[d == 0] = np.resize(np.array(EDGE_VALUES, np.float32), int((d == 0).sum()))
    rays = np.ascontiguousarray(np.concatenate([rays, edge]))
    assert len(rays) <= 75000
    rays.setflags(write=False)
    res = S.closest(rays, prims=S.brute_prims())
    surface = np.zeros(len(rays), bool)
    surface[N_RANDOM + N_AXIS:N_RANDOM + N_AXIS + N_SURFACE] = True
    return types.SimpleNamespace(name=name, scene=scene, S=S, rays=rays, res=res, surface=surface, large=not S.all_brute())


def _hit_normal(rec):
    return np.stack([rec["nx"], rec["ny"], rec["nz"]], axis=1).astype(np.float64)


def _yardstick(H, exact=None):
    """Per ray: the primitive and t64 the arm is held to, the statement's shading normal, and the clear rays.  A scene whose meshes the
    statement covers needs nothing else.  Elsewhere (`exact`: the exact arm's records of the same rays) a ray the exact arm sees hit a
    mesh above 2,000 triangles is held to the exact arm's record: t64 is NaN there, and it is clear when that hit is more than 1e-4
    max(1, |o|) from the origin, the statement's nearest other candidate more than 1e-4 relative behind it and its t resolved (`cond`, from
    the exact arm's normal); a ray on which the exact arm and the statement name different primitives otherwise is not clear."""
    res = H.res
    prim, t64, clear, normal = res["primitive"].copy(), res["t"].copy(), f64.clear(res), res["shading"].copy()
    if not H.large:
        return types.SimpleNamespace(primitive=prim, t=t64, t64=np.where(np.isfinite(t64), t64, np.nan), clear=clear, normal=normal, stated=prim >= 0)
    assert exact is not None
    S, rays = H.S, H.rays
    o, d = rays[:, 0:3].astype(np.float64), rays[:, 4:7].astype(np.float64)
    te, pe = exact["t"].astype(np.float64), exact["primitive"]
    big = np.isin(pe, [i for i in range(S.num_primitives) if not S.brute(i)])
    thr = f64.NEAR*np.maximum(1.0, np.abs(o).max(axis=1))
    scale = np.zeros(len(rays))
    for i in np.unique(pe[big]):
        pp, _, s = S.pose(int(i), rays[:, 3])
        c, rad = S.prims[int(i)].ball
        scale = np.where(pe == i, np.linalg.norm(pp, axis=1) + s*(np.linalg.norm(c) + rad), scale)
    with np.errstate(all="ignore"):
        cos = np.abs((_hit_normal(exact)*d).sum(axis=1))/np.linalg.norm(d, axis=1)
        cond = (np.linalg.norm(o, axis=1) + scale + te)/(te*cos)
        clear_big = big & (te > thr) & ((res["t"] - te) > f64.CLEAR*te) & (cond <= f64.COND) & ~res["near"]
    agree = ~big & (pe == prim)
    t = np.where(big, te, t64)
    return types.SimpleNamespace(primitive=np.where(big, pe, prim), t=t, t64=np.where(big | ~np.isfinite(t64), np.nan, t64),
                                 clear=np.where(big, clear_big, clear & agree), normal=np.where(big[:, None], _hit_normal(exact), normal), stated=~big & (prim >= 0))


def _share(H, Y):
    elsewhere = ~H.surface
    hit = np.isfinite(Y.t) & elsewhere
    clear = Y.clear & elsewhere
    print("CLEAR %-18s hit %6d  clear %6d  (%.1f %%)" % (H.name, int(hit.sum()), int(clear.sum()), 100.0*clear.sum()/max(1, hit.sum())))
    assert clear.sum() >= 0.85*hit.sum(), "%s: badly chosen rays: %d of %d hit rays are clear" % (H.name, int(clear.sum()), int(hit.sum()))
    assert hit.sum() >= 1000, H.name


# ---------------------------------------------------------------------------
# 2a: the clear rays are really clear -- host data alone (no GPU; a scene with a mesh above 2,000 triangles: inside 2b, from the exact arm)

@pytest.mark.parametrize("name", SCENES + ["glass"])
def test_most_hit_rays_are_clear_by_the_statement_alone(name):
    H = _host(name)
    if H.large:
        hit = np.isfinite(H.res["t"])
        assert hit.any()                                   # the statement's share of such a scene; the whole share is asserted in 2b
        return
    _share(H, _yardstick(H))
    # the rays at the slab test's edge are there, and hit something
    d = H.rays[-N_EDGE:, 4:7]
    for v in EDGE_VALUES:
        sel = (d.view(np.uint32) == v.view(np.uint32)).any(axis=1)
        assert sel.sum() >= N_EDGE//8 and np.isfinite(H.res["t"][-N_EDGE:][sel]).any(), (name, v)


# ---------------------------------------------------------------------------
# 2b - 2d: the default configuration

@functools.lru_cache(maxsize=None)
def _device(name):
    """both arms' closest-hit records of a scene's rays under the default configuration, and the yardstick"""
    H = _host(name)
    scene, r = trq._renderer(name)
    try:
        exact = r.trace_rays(H.rays)
        r.set_arithmetic(abi.ARITH_FAST)
        fast = r.trace_rays(H.rays)
        Y = _yardstick(H, exact)
        occ = {kind: r.trace_rays(_with_tmax(H.rays, Y.t, kind), "occluded") for kind in ("half", "more", "inf")}
    finally:
        r.close()
    return H, Y, exact, fast, occ


def _with_tmax(rays, t, kind):
    q = rays.copy()
    t32 = np.where(np.isfinite(t), t, 1.0).astype(np.float32)
    q[:, 7] = {"half": np.float32(0.5)*t32, "more": np.float32(1.5)*t32, "inf": np.full_like(t32, np.inf)}[kind]
    return q


def _check_primitive_and_occlusion(what, H, Y, fast, occ, sel=slice(None)):
    """2b on the rays `sel` of the scene's set"""
    clear, prim, t = Y.clear[sel], Y.primitive[sel], Y.t[sel]
    res = H.res
    differ = clear & (fast["primitive"] != prim)
    assert not differ.any(), "%s: %d of %d clear rays name another primitive than the statement (first: ray %d, %d against %d)" % (
        what, int(differ.sum()), int(clear.sum()), int(np.argmax(differ)), fast["primitive"][np.argmax(differ)], prim[np.argmax(differ)])
    clean_miss = (~np.isfinite(t) & ~res["near"][sel] & ~res["edge"][sel] & ~res["boxed"][sel]) if not H.large else np.zeros(len(t), bool)
    assert (fast["primitive"][clean_miss] == -1).all(), "%s: %d rays hit where the statement has nothing near" % (what, int((fast["primitive"][clean_miss] != -1).sum()))
    for kind, got in occ.items():
        tmax = _with_tmax(H.rays[sel], t, kind)[:, 7].astype(np.float64)
        with np.errstate(invalid="ignore"):
            decided = (clear & ~(np.abs(tmax - t) <= 1e-4*t)) | clean_miss
            want = (t < tmax)
        bad = decided & (got != want.astype(np.uint32))
        assert not bad.any(), "%s tmax=%s: %d of %d rays differ from t64 < tmax" % (what, kind, int(bad.sum()), int(decided.sum()))
        assert (got.sum() > 0 or kind == "half") and (got.sum() < len(got) or kind == "more"), (what, kind)


def _errors(H, Y, rec, sel=slice(None)):
    """|t - t64|/t64 and the angle to the statement's normal of the records `rec`, on the clear rays that have a t64"""
    use = Y.clear[sel] & np.isfinite(Y.t64[sel]) & (rec["primitive"] == Y.primitive[sel])
    t64 = Y.t64[sel][use]
    return use, np.abs(rec["t"][use].astype(np.float64) - t64)/t64, f64.angle(_hit_normal(rec)[use], Y.normal[sel][use])


@gpu
@pytest.mark.parametrize("name", SCENES)
def test_primitive_and_occlusion_on_clear_rays(name):
    H, Y, exact, fast, occ = _device(name)
    if H.large:
        _share(H, Y)
    _check_primitive_and_occlusion(name, H, Y, fast, occ)
    assert fast.tobytes() != exact.tobytes(), "%s: it really is another arithmetic" % name


@gpu
@pytest.mark.parametrize("name", SCENES)
def test_error_of_t_and_of_the_normal_against_float64(name):
    """Margins: isect_f64.error_margins (4x the exact arm's percentile, 16x its maximum), per scene and per primitive type of at least 200 rays."""
    H, Y, exact, fast, occ = _device(name)
    use, et_f, ea_f = _errors(H, Y, fast)
    use_e, et_e, ea_e = _errors(H, Y, exact)
    assert np.array_equal(use, use_e) and use.sum() >= 1000, name
    kinds = np.array([H.S.prims[p].type for p in Y.primitive[use]])
    for k, label in ((abi.GEOM_SPHERE, "sphere"), (abi.GEOM_PLANE, "plane"), (abi.GEOM_MESH, "triangle")):
        if (kinds == k).sum() >= 200:
            f64.error_margins("%s %s t" % (name, label), et_f[kinds == k], et_e[kinds == k])
            f64.error_margins("%s %s normal" % (name, label), ea_f[kinds == k], ea_e[kinds == k])
    same = float((fast["t"][use] == exact["t"][use]).mean())
    print("BITS  %-18s %.1f %% of the clear rays' t bit-equal to the exact arm's" % (name, 100*same))
    f64.error_margins("%s t" % name, et_f, et_e)
    f64.error_margins("%s normal" % name, ea_f, ea_e)
    if H.large:
        big = Y.clear & ~Y.stated & (fast["primitive"] == Y.primitive)
        rel = np.abs(fast["t"][big].astype(np.float64) - Y.t[big])/Y.t[big]
        print("LARGE %-18s |t_fast - t_exact|/t_exact over %d rays: median %.3e  99.9th %.3e  max %.3e" % (
            name, int(big.sum()), np.median(rel), np.percentile(rel, 99.9), rel.max()))
        assert big.sum() >= 50 and rel.max() <= LARGE_MESH_T, name


@functools.lru_cache(maxsize=None)
def _next_surface(name):
    """the statement's closest hit beyond the origin's zone (t > 1e-4 max(1, |o|)) of the rays that start on a surface"""
    H = _host(name)
    rays = H.rays[H.surface]
    thr = f64.NEAR*np.maximum(1.0, np.abs(rays[:, 0:3].astype(np.float64)).max(axis=1))
    return rays, thr, H.S.closest(rays, prims=H.S.brute_prims(), tmin=thr)


@gpu
@pytest.mark.parametrize("name", SCENES)
def test_rays_that_start_on_a_surface_flip_only_at_near_ties(name):
    """A ray that starts on a surface has that surface as a candidate at t = 0 +- rounding, and whether it is reported is a matter of a
    sign no arithmetic owns.  Counted are the rays on which the exact arm went on to the next surface (what the reference's table calls
    clear there) and that surface is clear by the statement: the tolerance arm may name another primitive on at most 1 % of the scene's
    hit rays -- and then only at a near-tie at the origin (isect_f64.near_tie: a primitive the statement places within 1e-4 max(1, |o|)
    of the origin, reported at such a t; or, leaving a sphere through its inside with a near root of exactly 0, what lies behind that
    sphere).  Anything else, the correct surface behind a lost one included, is a lost hit."""
    H, Y, exact, fast, occ = _device(name)
    S = H.S
    rays, thr, far = _next_surface(name)
    ex, fa = exact[H.surface], fast[H.surface]
    with np.errstate(invalid="ignore"):
        clear_far = np.isfinite(far["t"]) & (far["count"] == 1) & ((far["second"] - far["t"]) > f64.CLEAR*far["t"]) & ~far["edge"] & ~far["boxed"] & \
            (far["cond"] <= f64.COND)
    counted = clear_far & (ex["primitive"] == far["primitive"])
    flipped = counted & (fa["primitive"] != far["primitive"])
    hits = int(np.isfinite(Y.t).sum())
    print("FLIP  %-18s rays that start on a surface: the exact arm goes on to the statement's next surface on %d of %d, the tolerance arm names another "
          "primitive on %d of those (cap %d)" % (name, int(counted.sum()), len(rays), int(flipped.sum()), int(CAP*hits)))
    assert counted.sum() >= 50, name
    assert flipped.sum() <= CAP*hits, name
    sel = np.nonzero(flipped)[0]
    lost = list(sel[~f64.near_tie(S, rays[sel], far["primitive"][sel], fa["primitive"][sel], fa["t"][sel])])
    assert not lost, "%s: %d flipped rays report a primitive the statement places nowhere near (first: surface ray %d)" % (name, len(lost), lost[0])


# ---------------------------------------------------------------------------
# 2e: every pipeline and tuning arm

N_CONFIG = 8191


def _subset(H):
    """8,191 rays spread evenly over the scene's set: every block of it, the slab test's edge included"""
    idx = np.linspace(0, len(H.rays) - 1, N_CONFIG).astype(np.int64)
    assert len(np.unique(idx)) == N_CONFIG and N_CONFIG % 64 != 0 and (idx >= len(H.rays) - N_EDGE).sum() >= 100
    return idx


@gpu
@pytest.mark.parametrize("name", CONFIG_SCENES)
def test_every_pipeline_and_tuning_arm(name):
    H, Y, exact, fast, occ = _device(name)
    idx = _subset(H)
    rays = np.ascontiguousarray(H.rays[idx])
    queries = {kind: _with_tmax(rays, Y.t[idx], kind) for kind in ("half", "more", "inf")}
    base = fast[idx]

    def run(r, what):
        r.set_arithmetic(abi.ARITH_FAST)
        rec = r.trace_rays(rays)
        got = {kind: r.trace_rays(q, "occluded") for kind, q in queries.items()}
        _check_primitive_and_occlusion("%s %s" % (name, what), H, Y, rec, got, idx)
        same = int((rec.view(np.uint32).reshape(-1, 8) == base.view(np.uint32).reshape(-1, 8)).all(axis=1).sum())
        print("EQUAL %-18s %-36s %5d of %d records bit-equal to the default configuration's" % (name, what, same, len(rec)))
        if name in ("cornell", "ajax_standin_96"):
            use, et_f, ea_f = _errors(H, Y, rec, idx)
            use_e, et_e, ea_e = _errors(H, Y, exact[idx], idx)
            assert np.array_equal(use, use_e) and use.sum() >= 500
            f64.error_margins("%s %s t" % (name, what), et_f, et_e, quiet=True)
            f64.error_margins("%s %s normal" % (name, what), ea_f, ea_e, quiet=True)
            if H.large:
                big = Y.clear[idx] & ~Y.stated[idx] & (rec["primitive"] == Y.primitive[idx])
                rel = np.abs(rec["t"][big].astype(np.float64) - Y.t[idx][big])/Y.t[idx][big]
                assert big.sum() >= 50 and rel.max() <= LARGE_MESH_T, (name, what, rel.max())

    scene, r = trq._renderer(name)
    try:
        for label, pipe in PIPELINES.items():
            r.set_pipeline(pipe)
            run(r, "pipeline " + label)
    finally:
        r.close()
    for label, tuning in TUNINGS.items():
        r2 = tinsel_amd.HipRenderer(scene, 0, abi.Tuning(**tuning))
        try:
            run(r2, label)
        finally:
            r2.close()


# ---------------------------------------------------------------------------
# 3: radiance queries, per path and by depth
#
# radiance(starts, max_depth) on the 50 x 37 x 3 camera paths of tests/test_gpu_radiance_query._starts (the camera's own jittered paths: the
# raster positions need the reference's GenerateRay, so oracle/_ref), exact arm against tolerance arm on one renderer, depths 1, 2 and the
# pack's own.  A path is ON TRACK when max|d rgb| <= 1e-3 max(1e-3, max|rgb_exact|) (test_gpu_fast.py's rule).  A path leaves the track at a
# shadow or silhouette edge or a lobe choice: the off-track count does not fall with depth (slack: 5 paths); it is at most 4x the share the
# reference's own two builds (IEEE and -ffast-math, tests/golden/fast_yardstick.json, written by tests/golden/make_fast_yardstick.py) are
# off each other's track, plus 0.5 % of the paths -- 4x because this arm also gives up correctly rounded divides and glibc's sin / cos,
# which gcc -ffast-math keeps; and the off-track paths are other draws from the same distribution: with sigma the exact arm's per-path
# standard deviation of luminance, |sum fast - sum exact| <= 4 sqrt(2 n_off) sigma + 1e-3 sum |exact on-track|.

RADIANCE_SCENES = ["cornell", "veach", "features", "glass", "motionblur", "many_spheres", "cornell_probe", "ajax_standin_96"]
needs_ref = pytest.mark.skipif(not oa.have_ref(), reason="oracle/_ref not built")
YARDSTICK = os.path.join(oa.GOLDEN, "fast_yardstick.json")


def _luminance(rgb):
    return rgb[:, 0].astype(np.float64)*0.3 + rgb[:, 1].astype(np.float64)*0.6 + rgb[:, 2].astype(np.float64)*0.1


def off_track(exact, other):
    """the paths of `other` [n, 3] that left the track of `exact`"""
    return np.abs(other - exact).max(axis=-1) > 1e-3*np.maximum(1e-3, np.abs(exact).max(axis=-1))


def check_unbiased(what, exact, fast, off=None):
    """the three figures of one (scene, depth): off-track count, the difference of the luminance sums and its bound; asserts the bound"""
    off = off_track(exact, fast) if off is None else off
    le, lf = _luminance(exact), _luminance(fast)
    assert np.isfinite(fast).all(), what
    bound = 4.0*np.sqrt(2.0*off.sum())*le.std() + 1e-3*np.abs(le[~off]).sum()
    diff = abs(lf.sum() - le.sum())
    assert diff <= bound, "%s: the luminance sums differ by %.4e, bound %.4e (%d of %d paths off track)" % (what, diff, bound, int(off.sum()), len(off))
    return int(off.sum()), diff, bound


def _depths(own):
    return [("1", 1), ("2", 2), ("own", own)]


@functools.lru_cache(maxsize=None)
def _paths(name, pipeline="auto"):
    from tests.test_gpu_radiance_query import _case
    starts, _, own = _case(name)
    scene, r = trq._renderer(name)
    out = {}
    try:
        r.set_pipeline(PIPELINES[pipeline])
        for label, depth in (_depths(own) if pipeline == "auto" else [("2", 2)]):
            r.set_arithmetic(abi.ARITH_EXACT)
            e = r.radiance(starts, depth)[:, :3].copy()
            r.set_arithmetic(abi.ARITH_FAST)
            out[label] = (e, r.radiance(starts, depth)[:, :3].copy())
    finally:
        r.close()
    return out


def _check_paths(name, what, both, yard):
    counts = []
    for label, (e, f) in both.items():
        n_off, diff, bound = check_unbiased("%s depth %s" % (what, label), e, f)
        n = len(e)
        cap = 4.0*yard[label] + 0.005
        print("TRACK %-16s %-20s depth %-3s off track %4d of %d (%.3f %%; the reference's two builds %.3f %%, cap %.3f %%)  sums differ by %.3e, bound %.3e" % (
            name, what, label, n_off, n, 100.0*n_off/n, 100.0*yard[label], 100.0*cap, diff, bound))
        assert e.any() and not np.array_equal(e, f), (what, label)
        assert n_off <= cap*n, "%s depth %s: %d of %d paths off track, cap %.1f" % (what, label, n_off, n, cap*n)
        counts.append(n_off)
    for a, b in zip(counts, counts[1:]):
        assert a <= b + 5, "%s: the off-track count falls with depth: %s" % (what, counts)


@gpu
@needs_ref
@pytest.mark.parametrize("name", RADIANCE_SCENES)
def test_paths_stay_on_track_and_the_rest_is_unbiased(name):
    with open(YARDSTICK) as fh:
        yard = json.load(fh)["off_track_share"][name]
    _check_paths(name, "auto", _paths(name), yard)


@gpu
@needs_ref
@pytest.mark.parametrize("pipeline", ["wavefront", "megakernel", "split", "paired"])
@pytest.mark.parametrize("name", ["cornell", "glass", "ajax_standin_96"])
def test_paths_under_every_pipeline(name, pipeline):
    with open(YARDSTICK) as fh:
        yard = json.load(fh)["off_track_share"][name]
    _check_paths(name, pipeline, _paths(name, pipeline), yard)       # (the fifth, auto, at every depth: the test above)


def test_the_yardstick_file_covers_every_scene_and_depth():
    with open(YARDSTICK) as fh:
        yard = json.load(fh)
    assert (yard["width"], yard["height"], yard["passes"]) == (50, 37, 3)
    for name in RADIANCE_SCENES:
        row = yard["off_track_share"][name]
        assert set(row) == {"1", "2", "own"} and all(0.0 <= v <= 1.0 for v in row.values()), name


# ---------------------------------------------------------------------------
# 4: feature planes and gathers
#
# features(): 96 x 64, 4 passes, exact against tolerance arm.  w depends on camera samples only: rtol 1e-5.  Off the edge pixels -- those
# whose 3 x 3 neighbourhood in the exact arm's first_hit map holds more than one primitive, or a miss next to a hit, where a sample may fall on
# the other side -- albedo and normal are within 1e-4 max(|plane|, w), depth (sum of w t and of w t^2; the sum of w over the hits within 1e-5)
# within 1e-4 relative.  Edge pixels, from the exact arm alone (asserted under 35 %): cornell 12.4 %, features_probe 11.8 %,
# ajax_standin_96 4.5 %.

FEATURE_SCENES = ["cornell", "features_probe", "ajax_standin_96"]
FW, FH, FPASSES = 96, 64, 4


@gpu
@pytest.mark.parametrize("name", FEATURE_SCENES)
def test_feature_planes_follow_the_exact_arm_off_the_edges(name):
    scene, r = trq._renderer(name)
    cam, opt = trq._cam_opt(scene)
    opt.width, opt.height = FW, FH
    try:
        r.init(FW, FH)
        exact = r.features(cam, opt, 0, FPASSES)
        _, prim, _ = r.first_hit(cam, FW, FH)
        r.set_arithmetic(abi.ARITH_FAST)
        fast = r.features(cam, opt, 0, FPASSES)
    finally:
        r.close()
    pad = np.pad(prim, 1, mode="edge")
    nb = np.stack([pad[1 + dy:1 + dy + FH, 1 + dx:1 + dx + FW] for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    edge = (nb != prim[None]).any(axis=0)
    print("EDGES %-16s %.1f %% of the pixels are edge pixels" % (name, 100.0*edge.mean()))
    assert edge.mean() < 0.35 and (prim >= 0).any(), name
    assert list(fast) == list(exact) == list(abi.FEATURE_NAMES)
    inner = ~edge
    for n in abi.FEATURE_NAMES:
        e, f = exact[n].astype(np.float64), fast[n].astype(np.float64)
        assert fast[n].shape == (FH, FW, 4) and fast[n].dtype == np.float32 and np.isfinite(fast[n]).all(), (name, n)
        assert (fast[n][..., 3][exact[n][..., 3] > 0] > 0).all()
        np.testing.assert_allclose(f[..., 3], e[..., 3], rtol=1e-5, err_msg="%s %s w" % (name, n))
        if n == "depth":
            for c, tol in ((0, 1e-4), (1, 1e-4), (2, 1e-5)):
                rel = np.abs(f[..., c] - e[..., c])[inner]/np.maximum(np.abs(e[..., c])[inner], 1e-30)
                rel = np.where(e[..., c][inner] == f[..., c][inner], 0.0, rel)
                print("PLANE %-16s depth[%d] largest relative difference off the edges %.3e" % (name, c, rel.max()))
                assert rel.max() <= tol, (name, n, c)
        else:
            scale = np.maximum(np.abs(e[..., :3]).max(axis=-1), e[..., 3])
            rel = (np.abs(f[..., :3] - e[..., :3]).max(axis=-1)/np.maximum(scale, 1e-30))[inner & (scale > 0)]
            print("PLANE %-16s %-6s largest difference off the edges %.3e of max(|plane|, w)" % (name, n, rel.max()))
            assert rel.max() <= 1e-4, (name, n)
            assert (f[..., :3][inner & (scale == 0)] == 0).all()
    assert fast["depth"][..., 2].any() and any(not np.array_equal(fast[n], exact[n]) for n in abi.FEATURE_NAMES)


# gather / gather_sh: cornell, depth 1, 67 samples per point, both modes, exact against tolerance arm.  The draws do not depend on the
# arithmetic: the generator words of every start are bit-equal and the directions within 1e-5 rad; per point the means agree within
# section 3's bound on that point's 67 paths (n_off and sigma from radiance() on the starts each arm returned) -- for an SH coefficient
# times 0.64, the largest |Y_i| of bands 0 - 2.

G_SAMPLES, G_W, G_H = 67, 12, 9


@gpu
@pytest.mark.parametrize("mode", ["cosine", "sphere"])
def test_gathers_follow_the_exact_arm_point_by_point(mode):
    scene, r = trq._renderer("cornell")
    cam, opt = trq._cam_opt(scene)
    try:
        pts, t, prim, nrm = r.first_hit_points(cam, G_W, G_H)
        hit = (prim >= 0).ravel()
        points = tinsel_amd.gather_points(pts.reshape(-1, 3)[hit], nrm.reshape(-1, 3)[hit], G_SAMPLES, base_seed=4242)
        n = len(points)
        assert n >= 60
        out = {}
        for arith in (abi.ARITH_EXACT, abi.ARITH_FAST):
            r.set_arithmetic(arith)
            mean, starts = r.gather(points, G_SAMPLES, 1, mode, return_starts=True)
            sh, starts_sh = r.gather_sh(points, G_SAMPLES, 1, 2, mode, return_starts=True)
            assert starts.tobytes() == starts_sh.tobytes()
            out[arith] = (mean, sh, starts, r.radiance(starts, 1)[:, :3].copy())
    finally:
        r.close()
    (me, she, se, pe), (mf, shf, sf, pf) = out[abi.ARITH_EXACT], out[abi.ARITH_FAST]
    for k in ("rng1", "rng2", "time", "ox", "oy", "oz"):
        assert np.array_equal(se[k], sf[k]), k
    de = np.stack([se["dx"], se["dy"], se["dz"]], axis=1)
    df = np.stack([sf["dx"], sf["dy"], sf["dz"]], axis=1)
    ang = f64.angle(de, df)
    print("GATHER %-7s start directions: largest angle to the exact arm's %.3e rad" % (mode, ang.max()))
    assert ang.max() <= 1e-5 and np.abs(np.linalg.norm(df.astype(np.float64), axis=1) - 1.0).max() <= 1e-5
    off = off_track(pe, pf).reshape(n, G_SAMPLES)
    le = _luminance(pe).reshape(n, G_SAMPLES)
    bound = 4.0*np.sqrt(2.0*off.sum(axis=1))*le.std(axis=1) + 1e-3*np.where(off, 0.0, np.abs(le)).sum(axis=1)
    diff = np.abs(_luminance(mf[:, :3]) - _luminance(me[:, :3]))*G_SAMPLES
    print("GATHER %-7s %d points, %d of %d paths off track; largest difference of a point's sum against its bound: %.3f" % (
        mode, n, int(off.sum()), off.size, (diff/np.maximum(bound, 1e-30)).max()))
    assert np.isfinite(mf).all() and me.any() and (diff <= bound + 1e-12).all(), mode
    assert shf.shape == (n, 9, 4) and np.isfinite(shf).all()
    for i in range(9):
        d = np.abs(_luminance(shf[:, i, :3]) - _luminance(she[:, i, :3]))*G_SAMPLES
        assert (d <= 0.64*bound + 1e-12).all(), (mode, i)

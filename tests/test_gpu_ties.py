"""Exact ties on every traversal path of the HIP library, against the reference's Trace() (render.cpp:17-62).

The parity contract: strict `t < minT`, so of two hits with the same t the first VISITED wins -- and the visit
order is the reference's walk of its scene tree (and, inside a mesh, of its mesh tree).  Every path of the library keeps that promise by
a mechanism of its own (the flat scan's tie flag and re-trace, k_walk's record merge, k_swalk's ray replacement, k_step's merged walk,
the inline walks), and random rays meet an exact tie about never.  The corpus of tests/golden/make_ties.py feeds them directly: scenes
whose surfaces coincide, rays almost all of which tie, and what Trace() and PathTrace answered, recorded (the table is in
tests/test_ties.py, which also pins the two CPU checkers to the records).  Here every ray of every scene must come back with the
recorded primitive, t bits and normal bits -- there is no weaker class of rays -- under every pipeline and every tuning that selects
another traversal; the renders (whose later bounces and shadow rays tie as well) must give the recorded per-path radiance and
framebuffer bit for bit.  The one documented exception is measured, not assumed: under a device-built tree (rebuild_scene without
nodes, BVH_LBVH / BVH_PLOC) another visit order may name another member of the tied set, never another t.

kernel_times() names k_query and k_query_refill both "k_query" (the arm is plan_query's choice by the scene alone: beyond the flat
scan's 64 primitives it is the refill kernel, tn_host_query.h) and times k_swalk as the k_extend / k_shadow it replaces, told by its
work lists ("k_seg", as tests/test_gpu_mesh_scenes.py tells it)."""
import ctypes as C

import numpy as np
import pytest

from tinsel_amd import abi
from tests.golden import make_ties as mt
from tests.test_gpu_ray_query import TMAX_KINDS, _tmax
from tests.test_ties import FLT_MAX, corpus, port, same_bits  # noqa: F401  (port: a fixture)

pytestmark = pytest.mark.gpu

WAVEFRONT, MEGA, SPLIT, PAIRED, AUTO = (abi.PIPELINE_WAVEFRONT, abi.PIPELINE_MEGAKERNEL, abi.PIPELINE_WAVEFRONT_SPLIT,
                                        abi.PIPELINE_WAVEFRONT_PAIRED, abi.PIPELINE_AUTO)
PIPELINES = {"wavefront": WAVEFRONT, "megakernel": MEGA, "split": SPLIT, "paired": PAIRED, "auto": AUTO}
WALK_EVERYTHING = dict(walk_min_tris=0, small_mesh_bytes=0)
# tunings fixed when the renderer is made / per call: each selects another traversal somewhere (include/tinsel_hip.h)
CREATE_TUNINGS = [dict(flat_scan=0), dict(walk=0), WALK_EVERYTHING, dict(lds_scene=0)]
CALL_TUNINGS = [dict(scene_walk=0), dict(scene_walk=1), dict(quads_in_scan=0), dict(quads_in_scan=1), dict(walk_single=0), dict(walk_single=1)]


def _renderer(name, **tuning):
    import tinsel_amd
    scene = tinsel_amd.Scene(corpus().pack(name))
    return scene, tinsel_amd.create_gpu_renderer(scene, 0, abi.Tuning(**tuning) if tuning else None)


def _queries(name):
    return mt.query_rays(corpus().rows(name))


def _fields(rec):
    return rec["primitive"], rec["t"], np.stack([rec["nx"], rec["ny"], rec["nz"]], axis=1)


def _differing(name, rec):
    """rays whose record is not the recorded one, as (primitive, t, normal) counts -- every ray, every bit"""
    prim, t, nrm = corpus().records(name)
    gp, gt, gn = _fields(rec)
    assert not np.asarray(rec["reserved"]).any()
    return (int((gp != prim).sum()), int((gt.view(np.uint32) != t.view(np.uint32)).sum()),
            int((np.ascontiguousarray(gn).view(np.uint32) != nrm.view(np.uint32)).any(axis=1).sum()))


def _check_closest(name, rec, what):
    bad = _differing(name, rec)
    assert bad == (0, 0, 0), "%s, %s: rays that differ from Trace() in (primitive, t, normal): %s of %d" % (name, what, bad, len(rec))


def _occlusion(name, kind):
    prim, t, _ = corpus().records(name)
    tmin = np.where(prim >= 0, t, np.float32(np.inf)).astype(np.float32)
    q = _queries(name)
    q[:, 7] = _tmax(kind, tmin)
    with np.errstate(invalid="ignore"):
        return q, (tmin < q[:, 7]).astype(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------------
# closest hit on every ray, no weak class; occlusion

@pytest.mark.parametrize("name", mt.SCENES)
def test_closest_hit_and_occlusion_equal_trace_on_every_ray(name):
    scene, r = _renderer(name)
    try:
        rec = r.trace_rays(_queries(name), "closest")
        miss = rec["primitive"] < 0
        assert (rec["t"][miss] == FLT_MAX).all()
        _check_closest(name, rec, "default")
        for kind in TMAX_KINDS:
            q, want = _occlusion(name, kind)
            got = r.trace_rays(q, "occluded")
            assert np.array_equal(got, want), "%s tmax=%s: %d rays differ" % (name, kind, int((got != want).sum()))
    finally:
        r.close()


@pytest.mark.parametrize("group", ["pipelines", "create", "call", "call_walked"])
@pytest.mark.parametrize("name", mt.SCENES)
def test_every_traversal_path_resolves_ties_alike(name, group):
    """the same assertion under each pipeline setting and each tuning that selects another traversal"""
    q = _queries(name)
    qo, occ = _occlusion(name, "next")
    bad = []

    def ask(r, what):
        d = _differing(name, r.trace_rays(q, "closest"))
        o = int((r.trace_rays(qo, "occluded") != occ).sum())
        if d != (0, 0, 0) or o:
            bad.append((what, d, o))

    if group == "pipelines":
        scene, r = _renderer(name)
        try:
            for label, pipe in PIPELINES.items():
                r.set_pipeline(pipe)
                ask(r, label)
        finally:
            r.close()
    elif group == "create":
        for tuning in CREATE_TUNINGS:
            scene, r = _renderer(name, **tuning)
            try:
                ask(r, tuning)
            finally:
                r.close()
    else:
        base = WALK_EVERYTHING if group == "call_walked" else {}
        scene, r = _renderer(name, **base)
        try:
            for tuning in CALL_TUNINGS:
                r.set_tuning(abi.Tuning(**dict(base, **tuning)))
                for pipe in (AUTO, SPLIT):
                    r.set_pipeline(pipe)
                    ask(r, (tuning, pipe))
        finally:
            r.close()
    assert not bad, "%s: configurations that differ from Trace() (what, (primitive, t, normal) rays, occlusion rays): %s" % (name, bad)


# ---------------------------------------------------------------------------------------------------------------------------------
# renders: almost every first hit and most later hits tie -- k_bounce's re-trace, the shadow traces, k_walk's records, k_step's merged walk

def _render(name, pipeline, create=None, call=None, timing=False):
    scene, r = _renderer(name, **(create or {}))
    try:
        if call:
            r.set_tuning(abi.Tuning(**dict(create or {}, **call)))
        r.enable_kernel_timing(timing)
        r.set_pipeline(pipeline)
        cam, opt = abi.Camera.from_buffer_copy(scene.camera), abi.Options.from_buffer_copy(scene.options)
        r.init(opt.width, opt.height)
        r.set_pass_index(0)
        out = r.render(cam, opt, passes=mt.PASSES)
        rad = r.batch_radiance(mt.PASSES, opt.height, opt.width)
        return out, rad, (r.kernel_times() if timing else {}), r.walked_prims
    finally:
        r.close()


def _render_configs(pipeline):
    extra = [(WALK_EVERYTHING, None), (dict(flat_scan=0), None), (None, dict(scene_walk=0)), (WALK_EVERYTHING, dict(walk_single=0)),
             (None, dict(quads_in_scan=0))] if pipeline in (SPLIT, PAIRED) else [(WALK_EVERYTHING, None)]
    return [(None, None)] + extra


@pytest.mark.parametrize("pipeline", list(PIPELINES))
@pytest.mark.parametrize("name", mt.SCENES)
def test_renders_equal_the_recorded_passes(name, pipeline):
    c = corpus()
    want_rad, want_accum = c[name + "_radiance"], c[name + "_accum"]
    bad = []
    for create, call in _render_configs(PIPELINES[pipeline]):
        out, rad, _, _ = _render(name, PIPELINES[pipeline], create, call)
        paths = int((rad.view(np.uint32) != want_rad.view(np.uint32)).any(axis=-1).sum())
        if paths or not same_bits(out, want_accum):
            bad.append((create, call, paths))
    assert not bad, "%s %s: configurations that differ from the reference (create, call, paths of %d): %s" % (name, pipeline, want_rad[..., 0].size, bad)


def test_the_intended_kernels_ran():
    """one scene per kernel family"""
    # the fused k_bounce: the flat scan, its tie flag and the re-trace
    _, _, times, _ = _render("dup_flat", WAVEFRONT, timing=True)
    assert "k_bounce" in times, sorted(times)
    # k_walk / k_walk_rays: small meshes in HBM, walked ahead of the scan
    _, _, times, walked = _render("dup_walked", SPLIT, WALK_EVERYTHING, timing=True)
    assert walked > 1 and "k_walk" in times, (walked, sorted(times))
    _, _, times, walked = _render("dup_triangles", PAIRED, WALK_EVERYTHING, timing=True)
    assert walked >= 1 and "k_walk" in times and "k_step" in times, (walked, sorted(times))
    # k_swalk: a work list for every extension and shadow launch on top of the region ordering the scan kernels have too
    _, _, swalk, _ = _render("dup_scene_bvh", SPLIT, timing=True)
    _, _, inline, _ = _render("dup_scene_bvh", SPLIT, None, dict(scene_walk=0), timing=True)
    print("dup_scene_bvh, split: k_seg launches %d with k_swalk, %d with the inline walk" % (swalk.get("k_seg", (0,))[0], inline.get("k_seg", (0,))[0]))
    assert swalk.get("k_seg", (0,))[0] > inline.get("k_seg", (0,))[0] and "k_walk" not in swalk, (sorted(swalk), sorted(inline))
    # k_query (beyond the flat scan: plan_query's refill arm)
    scene, r = _renderer("dup_scene_bvh")
    try:
        assert scene.num_primitives > 64
        r.enable_kernel_timing(True)
        r.trace_rays(_queries("dup_scene_bvh"))
        times = r.kernel_times()
    finally:
        r.close()
    assert list(times) == ["k_query"] and times["k_query"][0] == 1, times


# ---------------------------------------------------------------------------------------------------------------------------------
# the other consumers of trace(): k_normals / trace_camera, k_features, k_cost -- on dup_flat

def test_first_hit_is_the_normals_frame_where_everything_ties(port):
    name = "dup_flat"
    scene, r = _renderer(name)
    h = port.load_pack(corpus().pack(name))
    try:
        cam, opt = abi.Camera.from_buffer_copy(scene.camera), abi.Options.from_buffer_copy(scene.options)
        W, H = opt.width, opt.height
        t, prim, nrm = r.first_hit(cam, W, H, time=1.0)
        hit = prim >= 0
        frame = np.zeros((H, W, 4), np.float32)
        frame[..., :3] = np.where(hit[..., None], nrm*np.float32(0.5) + np.float32(0.5), np.float32(0.0))
        frame[..., 3] = hit
        nopt = opt.copy()
        nopt.mode = abi.MODE_NORMALS
        assert same_bits(frame, port.render_normals(h, cam, nopt))
        r.init(W, H)
        assert same_bits(frame, r.render(cam, nopt, passes=1))
        # the camera rays of the corpus at time 1 (the even ones) are these pixels' rays: the recorded primitive
        rows = corpus().rows(name)
        first = mt.N_AIMED + mt.N_AXIS
        want = corpus().records(name)[0][first:first + W*H].reshape(H, W)
        even = (np.arange(W*H) % 2 == 0).reshape(H, W)
        assert rows[first, 6] == 1.0 and np.array_equal(prim[even], want[even])
        assert hit.sum() > W*H//2
    finally:
        port.free(h)
        r.close()


def test_feature_planes_name_the_winning_primitive(port):
    """albedo names the winner's material, normal its normal: the recorded Trace() on the beauty's own samples, accumulated in numpy"""
    from tests.accumulate_reference import add_passes
    from tests.test_gpu_features import _colours
    name, c = "dup_flat", corpus()
    scene, r = _renderer(name)
    try:
        cam, opt = abi.Camera.from_buffer_copy(scene.camera), abi.Options.from_buffer_copy(scene.options)
        W, H = opt.width, opt.height
        prim, t, nrm = c[name + "_beauty_prim"].astype(np.int32), c[name + "_beauty_t"], c[name + "_beauty_normal"]
        hit = prim >= 0
        colours = _colours(scene)
        assert len({tuple(colours[k]) for k in (0, 1)}) == 2 and len({tuple(colours[k]) for k in (2, 3)}) == 2        # (the duplicates differ in colour)
        paths = {n: np.zeros((len(prim), 4), np.float32) for n in abi.FEATURE_NAMES}
        paths["albedo"][hit, :3] = colours[prim[hit]]
        paths["normal"][hit, :3] = nrm[hit]
        paths["depth"][hit, 0], paths["depth"][hit, 1], paths["depth"][hit, 2] = t[hit], t[hit]*t[hit], np.float32(1.0)
        seeds = tuple(int(port.pass_seed(s)) for s in range(mt.PASSES))
        filt = (opt.filter.type, opt.filter.width, opt.filter.falloff, opt.filter.offset)
        r.init(W, H)
        got = r.features(cam, opt, 0, mt.PASSES)
        for n in abi.FEATURE_NAMES:
            want = add_passes(np.zeros((H, W, 4), np.float32), paths[n].reshape(mt.PASSES, H, W, 4), seeds, filt, np.inf)
            assert same_bits(got[n], want), "%s: %d pixels differ" % (n, int((got[n].view(np.uint32) != want.view(np.uint32)).any(axis=-1).sum()))
        assert hit.sum() > len(prim)//2
    finally:
        r.close()


def test_the_cost_map_counts_the_reference_walk_where_everything_ties(port):
    name = "dup_flat"
    scene, r = _renderer(name)
    h = port.load_pack(corpus().pack(name))
    try:
        cam, opt = abi.Camera.from_buffer_copy(scene.camera), abi.Options.from_buffer_copy(scene.options)
        r.init(opt.width, opt.height)
        m = r.render_cost(cam, opt, 0, mt.PASSES)
        keys = ("rays", "internal_visits", "tri_tests", "prim_tests")
        bad = []
        for j in range(opt.height):
            for i in range(opt.width):
                _, cnt, _ = port.render_seeded_counts(h, cam, opt, 0, mt.PASSES, window=(i, j, i + 1, j + 1), threads=1)
                if list(m[j, i]) != [cnt[k] for k in keys]:
                    bad.append(((i, j), list(m[j, i]), [cnt[k] for k in keys]))
        assert not bad, "%d pixels differ, first: %s" % (len(bad), bad[:3])
    finally:
        port.free(h)
        r.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# the mesh level: which of two triangles with the same t gives the normal

@pytest.mark.parametrize("where", ["arena", "hbm", "hbm_walked"])
def test_the_mesh_walk_picks_the_reference_trees_triangle(where):
    """dup_triangles' mesh through leaf(4, ...) -- PrimitiveIntersect on the device, the inline walk -- with the mesh in the LDS arena and in
    HBM: hit flag, t and the normal bits of the reference's PrimitiveIntersect (un-turned: before Trace()'s FaceForward)"""
    name, c = "dup_triangles", corpus()
    rows = c.rows(name)
    scene, r = _renderer(name, **{"arena": {}, "hbm": dict(small_mesh_bytes=0), "hbm_walked": WALK_EVERYTHING}[where])
    try:
        assert r.mesh_tree(1)[1]["inArena"] == (1 if where == "arena" else 0)
        out = r.leaf(4, 1, len(rows), 5, rows=rows)
    finally:
        r.close()
    hit = c[name + "_mesh_hit"] != 0
    assert np.array_equal(out[:, 0] > 0.5, hit)
    assert same_bits(out[hit, 1], c[name + "_mesh_t"][hit])
    differ = (np.ascontiguousarray(out[hit, 2:5]).view(np.uint32) != c[name + "_mesh_normal"][hit].view(np.uint32)).any(axis=1)
    assert not differ.any(), "%d of %d normals differ" % (int(differ.sum()), int(hit.sum()))
    assert (c[name + "_pair"] & hit).sum() >= mt.FLOOR_TIED


# ---------------------------------------------------------------------------------------------------------------------------------
# the documented exception, measured: device-built trees change the visit order, so the winner among EQUAL hits -- nothing else

def _check_member(name, rec, what):
    """t bit-equal on every ray, the primitive one of those that attain it; returns the number of winners that differ from Trace()'s"""
    c = corpus()
    prim, t, nrm = c.records(name)
    sets = c.tied_sets(name)
    gp, gt, gn = _fields(rec)
    ulps = np.abs(gt.view(np.int32).astype(np.int64) - t.view(np.int32).astype(np.int64))
    print("%s, %s: t differs on %d rays, at most %d ulp" % (name, what, int((ulps != 0).sum()), int(ulps.max())))
    assert not ulps.any(), "%s, %s: %d rays differ in t" % (name, what, int((ulps != 0).sum()))
    hit = prim >= 0
    assert np.array_equal(gp >= 0, hit)
    assert sets[np.nonzero(hit)[0], gp[hit]].all(), "%s, %s: a winner outside the tied set" % (name, what)
    other = gp != prim
    # where the winner is Trace()'s, so is the normal -- except inside a mesh, where the mesh tree may be the one that changed
    if not what.startswith("mesh"):
        assert same_bits(gn[~other], nrm[~other])
    return int(other.sum())


@pytest.mark.parametrize("name", ["dup_order", "dup_scene_bvh"])
def test_a_device_built_scene_tree_only_reorders_equal_hits(name):
    scene, r = _renderer(name)
    try:
        q = _queries(name)
        _check_closest(name, r.trace_rays(q), "the pack's tree")
        r.rebuild_scene()
        moved = _check_member(name, r.trace_rays(q), "scene tree built on the device")
        tied = int((corpus().tied_sets(name).sum(axis=1) > 1).sum())
        print("%s: device-built scene tree: %d of %d tied rays name another member of the tied set" % (name, moved, tied))
        d = scene.desc
        orig = (abi.BVHNode*d.num_bvh_nodes).from_buffer_copy(C.string_at(C.cast(d.bvh_nodes, C.c_void_p), d.num_bvh_nodes*C.sizeof(abi.BVHNode)))
        r.rebuild_scene(orig)
        _check_closest(name, r.trace_rays(q), "the pack's tree again")
    finally:
        r.close()


@pytest.mark.parametrize("mode", [abi.BVH_LBVH, abi.BVH_PLOC], ids=["lbvh", "ploc"])
@pytest.mark.parametrize("name", ["dup_walked", "dup_triangles"])
def test_device_built_mesh_trees_only_reorder_equal_hits(name, mode):
    c = corpus()
    scene, r = _renderer(name, small_mesh_bytes=0)
    try:
        q = _queries(name)
        _check_closest(name, r.trace_rays(q), "the pack's trees")
        r.set_mesh_bvh(mode)
        rec = r.trace_rays(q)
        moved = _check_member(name, rec, "mesh trees built on the device (mode %d)" % mode)
        prim, t, nrm = c.records(name)
        gn = _fields(rec)[2]
        differ = (np.ascontiguousarray(gn).view(np.uint32) != nrm.view(np.uint32)).any(axis=1)
        print("%s, mode %d: %d winners differ, %d normals differ" % (name, mode, moved, int(differ.sum())))
        if name == "dup_triangles":
            # a ray whose two triangles tie takes the normal of one of the two; every other ray Trace()'s -- but for the `contested` ones (the
            # generator's count, from the reference's PrimitiveIntersect on each triangle alone: ANOTHER triangle of the mesh has a hit within
            # 1e-5 |t|, equal included -- rays aimed at shared edges and vertices), where the first visited of two equal hits gives the normal
            # and which of two hits a few ulps apart survives MeshQuery's box cull (intersection.h:711-714) rests on the tree
            pair, contested = c[name + "_pair"], c[name + "_contested"]
            assert contested.sum() <= 0.01*pair.sum() and (pair & ~contested).sum() >= mt.FLOOR_TIED
            alt = (np.ascontiguousarray(gn).view(np.uint32) == c[name + "_alt_normal"].view(np.uint32)).all(axis=1)
            assert (~differ | alt)[pair & ~contested].all()
            assert not differ[~pair & ~contested].any(), "%d normals differ on rays that neither tie nor are contested" % int(differ[~pair & ~contested].sum())
            print("%s, mode %d: %d of %d tied rays take the other triangle's normal" % (name, mode, int((differ & pair).sum()), int(pair.sum())))
        r.set_mesh_bvh(abi.BVH_REFERENCE)
        _check_closest(name, r.trace_rays(q), "the pack's trees again")
    finally:
        r.close()

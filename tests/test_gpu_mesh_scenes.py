"""Mesh-heavy scenes (tests/golden/make_mesh_scenes.py: deep trees, 8+ mesh primitives, instanced meshes, a mesh light of thousands of
triangles, 65+ primitives with meshes in HBM) against the live reference: per-path radiance and framebuffer bit for bit under every pipeline
and, one at a time, every switch that moves a mesh walk to other code.

The scenes are generated at test time as .tin text, loaded by the reference's own loader + Scene::Build (oracle/_ref), written as a pack and
rendered by its PathTrace at 320 x 240, 2 passes.  Each family has to REACH the arm it was made for, shown from the library's own
introspection (walked_prims, kernel_times, mesh_tree, walk_tops), not assumed:

    one_big      1 walked primitive: k_walk with the tree as kernel arguments, and (walk_single = 0) with per-lane pointers
    seven        7 walked primitives whose tree tops do not all fit a workgroup's LDS: a later primitive stages less than its topCount
    twelve       7 walked primitives and 5 more walked inline by the scan kernels (the general variants)
    instances    16 primitives of 2 meshes, every third moving and turning: Moving64 poses on walked primitives
    mesh_light   a walked mesh of 2,000+ triangles is the emitter: a CDF search per light sample, shadow rays through k_walk
    beyond_flat  70-100 primitives: no flat scan, nothing for k_walk -- k_seg_* + k_swalk, meshes walked inline above the scene level

kernel_times() names k_walk and k_walk_rays both "k_walk", and times k_swalk as the k_extend / k_shadow it replaces; k_swalk's launches are
told by their work lists ("k_seg": k_seg_prefix + k_seg_expand_all before every launch, WITHOUT "k_walk", the only other user of such a list):
more "k_seg" launches than the same render with scene_walk = 0, which keeps only the ordering of the regions under that name.

A scene must not be vacuous.  From the reference's output alone (its frame, and its PrimitiveIntersect on the camera rays through the pixel
centres at time 0.5): radiance finite, at least half the pixels not black, at least 30 % of the camera rays end on a mesh primitive, and in
`twelve` at least 10 % on a mesh primitive from the eighth on.  The seeds below were chosen on the CPU to meet that; a seed that does not is
replaced, the condition stays.  `python -m tests.test_gpu_mesh_scenes` prints the table (prims, meshes, triangles of the largest mesh,
maxDepth, shadow rays per bounce as the light samples sum, the shares):

    family       seed prims meshes   tris depth  K    lit on mesh  late
    one_big         1     9      1  19880     6  1   0.86    0.64  0.00  ok
    one_big         2     8      1  19952     4  1   1.00    0.40  0.00  ok
    one_big         4     6      1  20000     3  3   0.79    0.61  0.00  ok
    seven           1     9      7   4756     4  3   0.90    0.46  0.00  ok
    seven           2    10      7   4356     6  6   1.00    0.32  0.00  ok
    seven           4    10      7   4648     6  2   0.84    0.43  0.00  ok
    twelve          1    15     12   5000     3  6   0.99    0.44  0.15  ok
    twelve          2    14     12   4970     3  2   1.00    0.41  0.17  ok
    twelve          3    15     12   4970     4  3   0.82    0.35  0.15  ok
    instances       1    19     16   3504     3  4   1.00    0.32  0.17  ok
    instances       2    19     16   2360     6  5   1.00    0.40  0.25  ok
    instances       3    19     16   3650     6  4   0.77    0.49  0.28  ok
    mesh_light      1     8      4   3128     4  3   0.99    0.41  0.00  ok
    mesh_light      2     8      4   3174     6  3   0.78    0.42  0.00  ok
    mesh_light      3     8      4   4970     4  2   1.00    0.51  0.00  ok
    beyond_flat     1    80      3   2928     3  4   1.00    0.41  0.00  ok
    beyond_flat     3    79     10   3813     6  5   0.94    0.47  0.15  ok
    beyond_flat     4    85      7   2548     3  2   0.98    0.51  0.00  ok
"""
import os
import tempfile

import numpy as np
import pytest

from tinsel_amd import abi
from tests import oracle_api as oa
from tests.golden import make_mesh_scenes as mm

needs_ref = pytest.mark.skipif(not oa.have_ref(), reason="oracle/_ref not built")

SEEDS = {"one_big": (1, 2, 4), "seven": (1, 2, 4), "twelve": (1, 2, 3), "instances": (1, 2, 3), "mesh_light": (1, 2, 3), "beyond_flat": (1, 3, 4)}
SCENES = [(f, s) for f in mm.FAMILIES for s in SEEDS[f]]
IDS = ["%s-%d" % c for c in SCENES]
PASSES = 2
THREADS = 16
WALK_EVERYTHING = dict(walk_min_tris=0, small_mesh_bytes=0)

SPLIT, PAIRED, AUTO = abi.PIPELINE_WAVEFRONT_SPLIT, abi.PIPELINE_WAVEFRONT_PAIRED, abi.PIPELINE_AUTO
TUNINGS = [{}, {"walk": 0}, {"walk_single": 0}, {"walk_lds_stack": 0}, {"walk_lds_stack": 2}, {"scene_walk": 0}, {"flat_scan": 0},
           {"quads_in_scan": 0}, {"batch_paths": 65536}, {"overlap": 1}]


# ---------------------------------------------------------------------------------------------------------------------------------
# the scenes and the reference's answers, made once per process

class Made:
    """a generated scene: pack bytes, the reference's handle (kept: conditions, ray tables), camera, options"""
    def __init__(self, R, family, seed, **kw):
        with tempfile.TemporaryDirectory() as d:
            tin = os.path.join(d, "%s_%d.tin" % (family, seed))
            with open(tin, "w") as fh:
                fh.write(mm.scene_text(family, seed, **kw))
            self.h = R.load_tin(tin)
            R.write_pack(self.h, tin + ".pack")
            with open(tin + ".pack", "rb") as fh:
                self.pack = fh.read()
        self.R, self.family, self.seed = R, family, seed
        self.cam, self.opt = R.camera_options(self.h)
        self.first_pass = 100*mm.FAMILIES.index(family) + seed
        self._frames = {}

    def frame(self, W=mm.WIDTH, H=mm.HEIGHT):
        """(camera, options, framebuffer, per-path radiance) of the reference at W x H"""
        if (W, H) not in self._frames:
            opt = abi.Options.from_buffer_copy(self.opt)
            opt.width, opt.height = W, H
            _default_float_environment()
            accum, rad, _ = self.R.render_seeded(self.h, self.cam, opt, self.first_pass, PASSES, want_accum=True, want_radiance=True, threads=THREADS)
            self._frames[(W, H)] = (self.cam, opt, accum, rad)
        return self._frames[(W, H)]


def _default_float_environment():
    """The reference must run in the IEEE environment it is compiled for.  oracle/_ref/libtinsel_ref_fast.so (the reference as its own makefile builds
    it, -ffast-math: tests/test_gpu_fast.py) switches the loading thread to flush-to-zero / denormals-are-zero when it is loaded, for the rest of the
    process, and the threads a later render starts inherit that.  No scene of the suite had a path near FLT_MIN before; mesh_light seed 1 has one
    (pass 0, pixel (36, 136): radiance 1.1893567e-37, with denormals flushed 1.1764619e-37), and beyond_flat seed 3 has filter weights there."""
    import ctypes
    libm = ctypes.CDLL("libm.so.6")
    libm.fesetenv.argtypes = [ctypes.c_void_p]
    assert libm.fesetenv(ctypes.c_void_p(-1)) == 0             # FE_DFL_ENV


_MADE = {}


def made(family, seed):
    if (family, seed) not in _MADE:
        if "R" not in _MADE:
            _MADE["R"] = oa.RefOracle()
        _MADE[(family, seed)] = Made(_MADE["R"], family, seed)
    return _MADE[(family, seed)]


def pack_bytes(name):
    """'mesh:FAMILY:SEED' -> the pack (tests/test_gpu_ray_query.py, tests/test_gpu_cost_map.py)"""
    if not oa.have_ref():
        pytest.skip("oracle/_ref not built: the mesh scenes are made by the reference's loader")
    _, family, seed = name.split(":")
    return made(family, int(seed)).pack


def conditions(m):
    """the table's row, from the reference alone"""
    R, h = m.R, m.h
    cam, opt, accum, rad = m.frame()
    W, H = opt.width, opt.height
    jj, ii = np.mgrid[0:H, 0:W]
    od = R.camera_rays(cam, W, H, np.stack([ii.ravel() + 0.5, jj.ravel() + 0.5], axis=1).astype(np.float32))
    rows = np.ascontiguousarray(np.concatenate([od, np.full((W*H, 1), 0.5, np.float32)], axis=1))
    best = np.full(W*H, np.inf, np.float32)
    prim = np.full(W*H, -1, np.int32)
    kinds = [R.primitive(h, p) for p in range(R.num_primitives(h))]
    for p in range(len(kinds)):
        hit, t, _ = R.primitive_intersect(h, p, rows)
        closer = (hit != 0) & (t > 0) & (t < best)
        best, prim = np.where(closer, t, best), np.where(closer, p, prim)
    mesh_prims = [p for p, k in enumerate(kinds) if k.type == abi.GEOM_MESH]
    tris = [kinds[p].geo.mesh.num_indices//3 for p in mesh_prims]
    late = mesh_prims[7:]
    return {"prims": len(kinds), "meshes": len(mesh_prims), "tris": max(tris), "depth": opt.max_depth,
            "K": sum(k.light_samples for k in kinds), "finite": bool(np.isfinite(rad).all() and np.isfinite(accum).all()),
            "lit": float((accum[..., :3] > 0).any(axis=-1).mean()), "on_mesh": float(np.isin(prim, mesh_prims).mean()),
            "late": float(np.isin(prim, late).mean()) if late else 0.0}


def check_conditions(m):
    c = conditions(m)
    assert c["finite"], c
    assert c["lit"] >= 0.5, c
    assert c["on_mesh"] >= 0.30, c
    if m.family == "twelve":
        assert c["late"] >= 0.10, c
    return c


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the plain-C restatement on the same scenes (k_cost's expected values rest on it; it had only ever seen 8-triangle meshes)

@needs_ref
@pytest.mark.skipif(not oa.have_port(), reason="oracle/libtinsel_oracle.so not built")
@pytest.mark.parametrize("family,seed", SCENES, ids=IDS)
def test_c_restatement_equals_the_reference_on_mesh_scenes(family, seed):
    m = made(family, seed)
    check_conditions(m)
    cam, opt, accum, rad = m.frame(96, 72)
    P = oa.PortOracle()
    h = P.load_pack(m.pack)
    accum2, rad2, _ = P.render_seeded(h, cam, opt, m.first_pass, PASSES, want_accum=True, want_radiance=True, threads=THREADS)
    P.free(h)
    differ = (rad != rad2).any(axis=-1)
    assert not differ.any(), "%s %d: %d paths differ, first (pass, row, column) %s" % (family, seed, int(differ.sum()), np.argwhere(differ)[0].tolist())
    assert np.array_equal(accum, accum2)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU

def _configs(family):
    pipes = [AUTO, SPLIT, PAIRED] + ([abi.PIPELINE_WAVEFRONT, abi.PIPELINE_MEGAKERNEL] if family in ("one_big", "instances") else [])
    return [(p, {}) for p in pipes] + [(p, t) for p in (SPLIT, PAIRED) for t in TUNINGS[1:]]


def _split_fields(tuning):
    create = {k: v for k, v in tuning.items() if k in abi.Tuning.CREATE_FIELDS}
    return create, {k: v for k, v in tuning.items() if k not in create}


def _expect_kernels(family, pipeline, tuning, times, walked):
    """what kernel_times() must list, by the arm the configuration asks for"""
    flat = family != "beyond_flat" and tuning.get("flat_scan", -1) != 0
    walking = flat and tuning.get("walk", -1) != 0
    if pipeline in (abi.PIPELINE_WAVEFRONT, abi.PIPELINE_MEGAKERNEL):
        assert ("k_bounce" if pipeline == abi.PIPELINE_WAVEFRONT else "k_mega") in times, times
        return
    assert walked == (0 if not walking else 1 if family == "one_big" else 7 if family in ("seven", "twelve", "instances") else walked), walked
    assert ("k_walk" in times) == (walked > 0), (walked, sorted(times))
    if pipeline == PAIRED and flat:
        assert "k_step" in times and "k_extend" not in times, sorted(times)
    if pipeline == SPLIT or not flat:
        assert "k_extend" in times and "k_shade" in times, sorted(times)
    if not flat:
        assert "k_seg" in times, sorted(times)


@pytest.mark.gpu
@needs_ref
@pytest.mark.parametrize("thresholds", [{}, WALK_EVERYTHING], ids=["default", "walk_everything"])
@pytest.mark.parametrize("family,seed", SCENES, ids=IDS)
def test_mesh_scenes_equal_the_reference(family, seed, thresholds):
    import tinsel_amd
    m = made(family, seed)
    check_conditions(m)
    cam, opt, accum, rad = m.frame()
    W, H = opt.width, opt.height
    scene = tinsel_amd.Scene(m.pack)
    bad, seen, renderers, seg = [], set(), {}, {}
    try:
        for pipeline, tuning in _configs(family):
            create, per_render = _split_fields(tuning)
            key = tuple(sorted(create.items()))
            if key not in renderers:
                renderers[key] = tinsel_amd.create_gpu_renderer(scene, 0, abi.Tuning(**dict(thresholds, **create)))
                renderers[key].enable_kernel_timing(True)
            r = renderers[key]
            r.set_tuning(abi.Tuning(**dict(thresholds, **tuning)))
            r.set_pipeline(pipeline)
            r.init(W, H)
            r.set_pass_index(m.first_pass)
            out = r.render(cam, opt, passes=PASSES)
            # (a batch limit below one pass: a batch per pass, the last one's paths are the ones still held)
            got = r.batch_radiance(1, H, W)[0] if "batch_paths" in tuning else r.batch_radiance(PASSES, H, W)
            want = rad[PASSES - 1] if "batch_paths" in tuning else rad
            times = r.kernel_times()               # (of this render call alone)
            _expect_kernels(family, pipeline, tuning, times, r.walked_prims)
            seen |= set(times)
            seg[(pipeline, tuple(sorted(tuning.items())))] = times.get("k_seg", (0,))[0]
            if not np.array_equal(got, want) or not np.array_equal(out, accum):
                differ = np.argwhere((got != want).any(axis=-1))
                bad.append((pipeline, tuning, len(differ), differ[0].tolist() if len(differ) else None))
        print("%s-%d %s: %s" % (family, seed, sorted(thresholds), " ".join(sorted(seen))))
        if family == "beyond_flat":
            # k_swalk's launches: a work list (k_seg_prefix + k_seg_expand_all) for every extension and every shadow launch, on top of the
            # region ordering that the scan kernels have too
            assert seg[(SPLIT, ())] > seg[(SPLIT, (("scene_walk", 0),))] > 0, seg
        renderers[()].set_tuning(abi.Tuning(**thresholds))
        _check_arm(family, scene, renderers[()])
    finally:
        for r in renderers.values():
            r.close()
    assert not bad, "%s %d: configurations that differ from the reference (pipeline, tuning, paths, first): %s" % (family, seed, bad)


@pytest.mark.gpu
@needs_ref
@pytest.mark.parametrize("pipeline", [SPLIT, PAIRED], ids=["split", "paired"])
def test_walk_records_that_would_number_2_31_fall_back_to_the_inline_walk(pipeline):
    """k_walk keeps one 32-byte closest-hit record per (ray, walked primitive) of a batch, by position, and needs fewer than 2^31 of them
    (plan_batch: capacity x rays per position x walked primitives; K rays per position in the split pipeline, K + 1 in the paired one).
    A batch beyond that is rendered with every mesh walked inline -- silently, so this is the only place that sees it happen.

    The scene: `seven` seed 1 with the most lights the generator gives (3 lights x 3 samples: K = 9, read back from nee_per_path), maxDepth 2.
    A batch is a whole number of passes, so one pass cannot be cut to make the records fit; the frame is 1600 x 1200 and the render as many passes as
    bring ONE batch over 2^31 records (18 split, 16 paired: 34.6 M / 30.7 M paths), rendered again with batch_paths = 2 passes (3.84 M paths, 242 M /
    269 M records).  The two framebuffers must be equal bit for bit, k_walk must be in the second render's kernel_times() and not in the first's,
    and the same scene at 320 x 240 must equal the reference.  Device memory while the large batch is held (path state, shadow rays, radiance):
    12.8 GB in the split pipeline, 34.2 GB in the paired one; both pipelines together take under 10 s on an MI355X."""
    import tinsel_amd
    import torch
    m = Made(made("seven", 1).R, "seven", 1, most_lights=True)
    try:
        scene = tinsel_amd.Scene(m.pack)
        r = tinsel_amd.create_gpu_renderer(scene)
        r.set_pipeline(pipeline)
        r.enable_kernel_timing(True)
        assert r.walked_prims == 7
        K = r.nee_per_path
        assert K == mm.MAX_LIGHTS*mm.MAX_LIGHT_SAMPLES
        # as in section 2: the reference at 320 x 240
        cam, opt, accum, rad = m.frame()
        r.init(opt.width, opt.height)
        r.set_pass_index(m.first_pass)
        out = r.render(cam, opt, passes=PASSES)
        assert "k_walk" in r.kernel_times()
        assert np.array_equal(r.batch_radiance(PASSES, opt.height, opt.width), rad) and np.array_equal(out, accum)
        # the large batch
        big = abi.Options.from_buffer_copy(m.opt)
        big.width, big.height, big.max_depth = 1600, 1200, 2
        per_pass = big.width*big.height
        rays = K if pipeline == SPLIT else K + 1
        passes = -(-2**31//(per_pass*rays*7))
        assert per_pass*passes*rays*7 >= 2**31 and per_pass*passes <= 64 << 20 and per_pass*2*rays*7 < 2**31
        free0 = torch.cuda.mem_get_info()[0]
        r.init(big.width, big.height)
        r.set_pass_index(0)
        whole = r.render(cam, big, passes=passes)
        times_whole = r.kernel_times()
        print("pipeline %d: %d passes, %.1f M paths in one batch, %.2f GB of device memory" % (pipeline, passes, per_pass*passes/1e6,
                                                                                              (free0 - torch.cuda.mem_get_info()[0])/1e9))
        r.set_tuning(batch_paths=2*per_pass)
        r.init(big.width, big.height)
        r.set_pass_index(0)
        cut = r.render(cam, big, passes=passes)
        times_cut = r.kernel_times()
        r.close()
        assert "k_walk" not in times_whole and ("k_extend" in times_whole or "k_step" in times_whole), sorted(times_whole)
        assert "k_walk" in times_cut, sorted(times_cut)
        assert np.isfinite(whole).all() and (whole[..., :3] > 0).any(axis=-1).mean() >= 0.5
        assert np.array_equal(whole, cut), "%d pixels differ" % int((whole != cut).any(axis=-1).sum())
    finally:
        m.R.free(m.h)


def _check_arm(family, scene, r):
    """the trees and the plan of the renderer with the default switches"""
    prims = C_prims(scene)
    mesh_prims = [p for p, k in enumerate(prims) if k.type == abi.GEOM_MESH]
    metas = {p: r.mesh_tree(p)[1] for p in mesh_prims}
    assert all(not v["inArena"] for v in metas.values())               # every mesh has 9 triangles or more: none rides in the arena
    if family == "beyond_flat":
        assert r.walked_prims == 0 and scene.num_primitives > 64
        assert max(v["stackNeed"] for v in metas.values()) > 8
        return
    walked = mesh_prims[:7]
    assert r.walked_prims == len(walked) == {"one_big": 1, "mesh_light": len(mesh_prims)}.get(family, 7)
    # a tree deeper than the 8 entries of the default LDS stack: its walk spills to the HBM part
    assert max(metas[p]["stackNeed"] for p in walked) > 8, metas
    tops = r.walk_tops()
    assert len(tops) == len(walked) and all(0 <= t <= metas[p]["topCount"] for t, p in zip(tops, walked))
    if family == "mesh_light":
        light = [p for p in mesh_prims if prims[p].light_samples > 0]
        assert len(light) == 1 and light[0] in walked and metas[light[0]]["numTris"] >= 2000
    if family == "instances":
        assert len(mesh_prims) == 16 and len({prims[p].geo.mesh.id for p in mesh_prims}) == 2
        moving = [p for p in walked if bytes(prims[p].start_transform) != bytes(prims[p].end_transform)]
        assert len(moving) >= 2, moving
    if family == "twelve":
        assert len(mesh_prims) == 12
    if family == "seven":
        assert any(metas[p]["topCount"] < metas[p]["numInternal"] for p in walked), metas
        # the tops compete for what the stacks leave of the LDS, handed out in primitive order: someone gets less than its top
        assert sum(tops) < sum(metas[p]["topCount"] for p in walked), (tops, metas)
        assert tops[0] > 0 and any(t < metas[p]["topCount"] for t, p in zip(tops, walked))


def C_prims(scene):
    import ctypes as C
    arr = C.cast(scene.desc.primitives, C.POINTER(abi.Primitive))
    return [arr[p] for p in range(scene.desc.num_primitives)]


if __name__ == "__main__":
    # the table of the module docstring (no GPU)
    print("    %-12s %4s %5s %6s %6s %5s %2s  %5s %7s %5s" % ("family", "seed", "prims", "meshes", "tris", "depth", "K", "lit", "on mesh", "late"))
    for family, seed in SCENES:
        m = made(family, seed)
        c = conditions(m)
        ok = c["finite"] and c["lit"] >= 0.5 and c["on_mesh"] >= 0.3 and (family != "twelve" or c["late"] >= 0.1)
        print("    %-12s %4d %5d %6d %6d %5d %2d  %5.2f %7.2f %5.2f  %s" % (family, seed, c["prims"], c["meshes"], c["tris"], c["depth"], c["K"], c["lit"],
                                                                          c["on_mesh"], c["late"], "ok" if ok else "REPLACE THE SEED"), flush=True)

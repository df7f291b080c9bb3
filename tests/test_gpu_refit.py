"""tinsel_hip_refit_mesh: new vertex positions for a mesh whose topology did not change (deforming / animated meshes;
the reference re-runs its host SAH build for that, mesh.cpp:314-338, and Scene::Build, scene.cpp:4-16).  The trees keep their
shape and every box is recomputed bottom-up: the mesh's own tree on the device, and at the SCENE level the leaf box of every
instance (PrimitiveBounds, intersection.h:906-939) and its ancestors in the scene BVH.

Oracle: the SAME displaced mesh inside a scene pack whose reference BVH nodes were refitted here on the host with numpy
(leaf box = min/max of the triangle's vertices, node box = union of the children's: what Bounds::AddPoint / the builder
store -- min and max do not round), whose area CDF follows Mesh::RebuildCDF's serial order and whose SCENE BVH was refitted
too (leaf box = the oracle's PrimitiveBounds of the refitted mesh -- pinned to the reference's in tests/test_oracle.py --
ancestors = union of their children), rendered by the C oracle on the CPU.  Same trees, same boxes, same triangles => the
GPU must be bit-identical to it.  The displacements leave the original bounds: with stale scene-level boxes the mesh would
be clipped (asserted: the oracle itself renders another image with the stale boxes)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from tinsel_amd import abi
from tests import oracle_api as oa
from tests import refit_host as rh
# the host refit of a pack lives in tests/refit_host.py (pinned to the reference's builder on the CPU: tests/test_refit_host.py)
from tests.refit_host import mesh_views as _mesh_views, refit_pack as _refit_pack
from tests.test_gpu_parity import _load

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not oa.have_ref(), reason="oracle/_ref not built: the mesh scenes are made by the reference's loader")


def _displace(pos, amount):
    p = pos.astype(np.float32).copy()
    p[:, 1] += (amount*np.sin(7.0*p[:, 0].astype(np.float64) + 3.0*p[:, 2].astype(np.float64))).astype(np.float32)
    p[:, 0] *= np.float32(1.0 + 4.0*amount)          # 20 % wider: well outside the original leaf box
    return p


def _mesh_prim(scene):
    prims = C.cast(scene.desc.primitives, C.POINTER(abi.Primitive))
    return [i for i in range(scene.desc.num_primitives) if prims[i].type == abi.GEOM_MESH][0]


@pytest.mark.parametrize("bvh", [abi.BVH_REFERENCE, abi.BVH_LBVH], ids=["reference-tree", "device-built-tree"])
def test_refit_after_displacement_matches_the_oracle_on_the_refitted_pack(bvh):
    import tinsel_amd
    name = "ajax_standin_96"                                        # 18,432 triangles, in HBM, walked by k_walk
    scene, cam, opt, g = _load(name)
    passes = 2
    blob = bytearray(open(os.path.join(oa.GOLDEN, name + ".pack"), "rb").read())
    prim = _mesh_prim(scene)
    old_pos = _mesh_views(blob, prim)[0].copy()
    new_pos = _displace(old_pos, 0.05)
    _refit_pack(blob, prim, new_pos)

    P = oa.PortOracle()
    h = P.load_pack(bytes(blob))
    ref_accum, ref_rad, _ = P.render_seeded(h, cam, opt, 0, passes, want_radiance=True)
    P.free(h)
    assert not np.array_equal(ref_rad, g["radiance"][:passes])      # the displacement is visible
    # ... and it leaves the original bounds: with the scene BVH as loaded (stale leaf box) the oracle itself clips the mesh
    stale = bytearray(open(os.path.join(oa.GOLDEN, name + ".pack"), "rb").read())
    _refit_pack(stale, prim, new_pos, scene_level=False)
    h = P.load_pack(bytes(stale))
    _, stale_rad, _ = P.render_seeded(h, cam, opt, 0, passes, want_radiance=True)
    P.free(h)
    assert not np.array_equal(stale_rad, ref_rad)

    r = tinsel_amd.create_gpu_renderer(scene)
    if bvh == abi.BVH_LBVH:
        r.set_mesh_bvh(abi.BVH_LBVH)
    r.refit_mesh(prim, new_pos)
    r.set_pipeline(abi.PIPELINE_WAVEFRONT_SPLIT)
    r.init(opt.width, opt.height)
    out = r.render(cam, opt, passes=passes)
    rad = r.batch_radiance(passes, opt.height, opt.width)
    same = float((rad == ref_rad).all(axis=-1).mean())
    if bvh == abi.BVH_REFERENCE:
        assert np.array_equal(rad, ref_rad), "%.4f %% of the paths identical" % (100*same)
        assert np.array_equal(out, ref_accum)
    else:
        assert same >= 0.999 and oa.image_l2(out, ref_accum) <= 1e-3    # another tree shape: exact-t ties may resolve differently
        # back to the reference's tree: it was refitted too
        r.set_mesh_bvh(abi.BVH_REFERENCE)
        r.init(opt.width, opt.height); r.set_pass_index(0)
        assert np.array_equal(r.render(cam, opt, passes=passes), ref_accum)
    # refit back to the original vertices restores the original image bit for bit
    r.refit_mesh(prim, old_pos)
    r.init(opt.width, opt.height); r.set_pass_index(0)
    assert np.array_equal(r.render(cam, opt, passes=int(g["passes"])), g["accum"])
    r.close()


def test_refit_of_a_light_mesh_updates_cdf_and_area(monkeypatch):
    """cornell's quad light as a mesh in HBM (tinsel_hip_tuning::small_mesh_bytes = 0): moving its vertices changes the light's area
    (PrimitiveArea -> the light pdf) and its sampling CDF; the oracle renders the refitted pack."""
    import tinsel_amd
    from tinsel_amd import renderer
    monkeypatch.setattr(renderer, "DEFAULT_TUNING", abi.Tuning(small_mesh_bytes=0))
    scene, cam, opt, g = _load("cornell")
    blob = bytearray(open(os.path.join(oa.GOLDEN, "cornell.pack"), "rb").read())
    prim = _mesh_prim(scene)
    pos = _mesh_views(blob, prim)[0].copy()
    new_pos = pos.copy()
    new_pos[:, 0] *= np.float32(1.6)                 # a wider light (it leaves its old box)
    new_pos[0, 2] += np.float32(0.05)                # and no longer a parallelogram: the two triangles differ in area
    _refit_pack(blob, prim, new_pos)
    P = oa.PortOracle()
    h = P.load_pack(bytes(blob))
    ref_accum, ref_rad, _ = P.render_seeded(h, cam, opt, 0, 2, want_radiance=True)
    P.free(h)
    r = tinsel_amd.create_gpu_renderer(scene)
    r.refit_mesh(prim, new_pos)
    r.init(opt.width, opt.height)
    out = r.render(cam, opt, passes=2)
    rad = r.batch_radiance(2, opt.height, opt.width)
    r.close()
    assert np.array_equal(rad, ref_rad), "%d paths differ" % int((rad != ref_rad).any(axis=-1).sum())
    assert np.array_equal(out, ref_accum)


def test_refit_of_a_mesh_in_the_lds_arena():
    """cornell as shipped: the quad light rides in the LDS-staged scene arena (fused kernel, the two-leaf walk).  The refit
    rewrites its records in the arena's copy in HBM, which every launch stages from."""
    import tinsel_amd
    scene, cam, opt, g = _load("cornell")
    blob = bytearray(open(os.path.join(oa.GOLDEN, "cornell.pack"), "rb").read())
    prim = _mesh_prim(scene)
    pos = _mesh_views(blob, prim)[0].copy()
    new_pos = pos.copy()
    new_pos[:, 0] *= np.float32(1.7)                 # a wider light: leaves its old box
    new_pos[0, 2] += np.float32(0.05)
    _refit_pack(blob, prim, new_pos)
    P = oa.PortOracle()
    h = P.load_pack(bytes(blob))
    ref_accum, ref_rad, _ = P.render_seeded(h, cam, opt, 0, 2, want_radiance=True)
    P.free(h)
    r = tinsel_amd.create_gpu_renderer(scene)
    r.refit_mesh(prim, new_pos)
    r.init(opt.width, opt.height)
    out = r.render(cam, opt, passes=2)
    rad = r.batch_radiance(2, opt.height, opt.width)
    assert np.array_equal(rad, ref_rad), "%d paths differ" % int((rad != ref_rad).any(axis=-1).sum())
    assert np.array_equal(out, ref_accum)
    r.refit_mesh(prim, pos)                          # and back
    r.init(opt.width, opt.height); r.set_pass_index(0)
    assert np.array_equal(r.render(cam, opt, passes=int(g["passes"])), g["accum"])
    r.close()


def test_refit_refuses_what_it_cannot_do():
    import tinsel_amd
    scene, cam, opt, g = _load("cornell")
    r = tinsel_amd.create_gpu_renderer(scene)
    prim = _mesh_prim(scene)
    with pytest.raises(tinsel_amd.TinselHipError):
        r.refit_mesh(0 if prim != 0 else 1, np.zeros((4, 3), np.float32))      # not a mesh
    r.close()
    scene, cam, opt, g = _load("ajax_standin_96")
    r = tinsel_amd.create_gpu_renderer(scene)
    with pytest.raises(tinsel_amd.TinselHipError, match="topology"):
        r.refit_mesh(_mesh_prim(scene), np.zeros((5, 3), np.float32))
    r.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# Beyond one mesh with one static instance and positions only: vertex normals, instanced and moving meshes, a large mesh light with
# zero-area triangles, and what follows a refit (device builds, scene rebuilds, further refits, queries).  Frames are 96 x 72 with
# 2 passes unless a fixture's own golden is compared.  The oracle is PortOracle on the host-refitted pack and, where oracle/_ref is
# there, the reference itself on the same bytes: the two must agree bit for bit before the GPU is looked at.  Every test first shows
# ON THE ORACLE that it has teeth: the refit changes the image, and so does each thing the refit could forget (stale scene-level
# leaves, the old normals, the old area).  Reference trees: np.array_equal.  Device-built trees (another tree shape resolves exact-t
# ties differently): >= 99.9 % of the paths bit-identical and image_l2 <= 1e-3, and bit-identical again back on the reference trees.

W, H, PASSES = 96, 72, 2
AUTO, SPLIT, PAIRED = abi.PIPELINE_AUTO, abi.PIPELINE_WAVEFRONT_SPLIT, abi.PIPELINE_WAVEFRONT_PAIRED


@functools.lru_cache(None)
def _ref():
    return oa.RefOracle()


def _small(opt):
    o = opt.copy()
    o.width, o.height = W, H
    return o


def _oracle(blob, cam, opt, first_pass=0, passes=PASSES):
    """(accumulator, per-path radiance) of the C oracle on pack bytes; the reference's own PathTrace on the same bytes must agree"""
    from tests.test_gpu_mesh_scenes import _default_float_environment
    _default_float_environment()
    P = oa.PortOracle()
    h = P.load_pack(bytes(blob))
    accum, rad, _ = P.render_seeded(h, cam, opt, first_pass, passes, want_radiance=True, threads=16)
    P.free(h)
    if oa.have_ref():
        h = _ref().load_pack(bytes(blob))
        accum2, rad2, _ = _ref().render_seeded(h, cam, opt, first_pass, passes, want_radiance=True, threads=16)
        _ref().free(h)
        assert np.array_equal(rad, rad2) and np.array_equal(accum, accum2), "the two oracles differ on the refitted pack"
    return accum, rad


def _differ(a, b):
    """two oracle results (accumulator, radiance) are different images"""
    return not np.array_equal(a[1], b[1])


def _refitted(original, prim, pos, normals=None, scene_level=True):
    blob = bytearray(original)
    _refit_pack(blob, prim, pos, normals, scene_level)
    return blob


def _gpu(r, cam, opt, first_pass=0, passes=PASSES):
    r.init(opt.width, opt.height)
    r.set_pass_index(first_pass)
    out = r.render(cam, opt, passes=passes)
    return out, r.batch_radiance(passes, opt.height, opt.width)


def _exact(got, want, what):
    differ = (got[1] != want[1]).any(axis=-1)
    assert np.array_equal(got[1], want[1]), "%s: %d of %d paths differ from the oracle" % (what, int(differ.sum()), differ.size)
    assert np.array_equal(got[0], want[0]), "%s: the accumulator differs" % what


def _device_tree_bars(got, want, what):
    same = float((got[1] == want[1]).all(axis=-1).mean())
    l2 = oa.image_l2(got[0], want[0])
    print("%s: %.4f %% of the paths identical to the oracle, L2 %.3e" % (what, 100*same, l2))
    assert same >= 0.999 and l2 <= 1e-3, what


def _new_normals(normals, seed):
    """unit normals perturbed by N(0, 0.3^2) per component, renormalised in fp32"""
    n = (normals + np.random.default_rng(seed).normal(0.0, 0.3, normals.shape)).astype(np.float32)
    ln = np.sqrt((n[:, 0]*n[:, 0] + n[:, 1]*n[:, 1]) + n[:, 2]*n[:, 2])
    assert ln.dtype == np.float32 and (ln > 0).all()
    return (n/ln[:, None]).astype(np.float32)


def _golden_pack(name):
    with open(os.path.join(oa.GOLDEN, name + ".pack"), "rb") as fh:
        return fh.read()


# -- normals ------------------------------------------------------------------------------------------------------------------------

def test_refit_with_normals_matches_the_oracle():
    """ajax_standin_96 (18,432 triangles, HBM, walked): positions + normals, normals alone, positions alone (the normals stay), and back"""
    import tinsel_amd
    name = "ajax_standin_96"
    scene, cam, gopt, g = _load(name)
    opt = _small(gopt)
    original = _golden_pack(name)
    prim = _mesh_prim(scene)
    pos0, nrm0 = _mesh_views(bytearray(original), prim)[0].copy(), rh.mesh_normals(bytearray(original), prim).copy()
    pos1, pos3 = _displace(pos0, 0.05), _displace(pos0, 0.03)
    nrm1, nrm2 = _new_normals(nrm0, 1), _new_normals(nrm0, 2)
    want = lambda pos, nrm, scene_level=True: _oracle(_refitted(original, prim, pos, nrm, scene_level), cam, opt)
    before = _oracle(original, cam, opt)
    want1, want2, want3 = want(pos1, nrm1), want(pos1, nrm2), want(pos3, nrm2)
    assert _differ(want1, before) and _differ(want1, want(pos1, nrm1, False)) and _differ(want1, want(pos1, nrm0))
    assert _differ(want2, want1)
    assert _differ(want3, want2) and _differ(want3, want(pos3, nrm0)) and _differ(want3, want(pos3, nrm1))
    changed = float((want(pos0, nrm1)[1] != before[1]).any(axis=-1).mean())
    print("normals alone change %.1f %% of the paths" % (100*changed))
    assert changed > 0.05

    r = tinsel_amd.create_gpu_renderer(scene)
    assert not r.mesh_tree(prim)[1]["inArena"]
    r.refit_mesh(prim, pos1, nrm1)
    _exact(_gpu(r, cam, opt), want1, "positions and normals")
    r.refit_mesh(prim, pos1, nrm2)
    _exact(_gpu(r, cam, opt), want2, "normals, the positions unchanged")
    r.refit_mesh(prim, pos3)
    _exact(_gpu(r, cam, opt), want3, "positions alone: the normals are kept")
    r.refit_mesh(prim, pos0, nrm0)
    out, rad = _gpu(r, cam, gopt, 0, int(g["passes"]))
    r.close()
    assert np.array_equal(rad, g["radiance"]) and np.array_equal(out, g["accum"])


def test_refit_normals_of_a_mesh_in_the_lds_arena():
    """glass with the default tuning: its small meshes ride in the LDS-staged arena, whose HBM copy holds their normals too"""
    import tinsel_amd
    name = "glass"
    scene, cam, gopt, g = _load(name)
    opt = _small(gopt)
    original = _golden_pack(name)
    before = _oracle(original, cam, opt)
    r = tinsel_amd.create_gpu_renderer(scene)
    tris = lambda p: len(_mesh_views(bytearray(original), p)[1])
    arena = sorted((p for p in rh.mesh_prims(original) if r.mesh_tree(p)[1]["inArena"]), key=tris, reverse=True)
    picked = None
    # the largest one whose vertex normals shade (of glass's three meshes the default tuning takes only the 2-triangle quad into the arena,
    # mesh_tree says; the 12-triangle cube and the sphere stay in HBM)
    for p in arena:
        pos0, nrm0 = _mesh_views(bytearray(original), p)[0].copy(), rh.mesh_normals(bytearray(original), p).copy()
        nrm1 = _new_normals(nrm0, 3)
        want1 = _oracle(_refitted(original, p, pos0, nrm1), cam, opt)
        if _differ(want1, before):
            picked = p
            break
    assert picked is not None, arena
    prim = picked
    print("arena meshes %s, refitted: primitive %d of %d triangles" % (arena, prim, tris(prim)))
    pos1 = _displace(pos0, 0.05)
    want2 = _oracle(_refitted(original, prim, pos1, nrm1), cam, opt)
    assert _differ(want2, want1) and _differ(want2, _oracle(_refitted(original, prim, pos1, nrm0), cam, opt))
    assert _differ(want2, _oracle(_refitted(original, prim, pos1, nrm1, False), cam, opt))
    r.refit_mesh(prim, pos0, nrm1)
    _exact(_gpu(r, cam, opt), want1, "normals of an arena mesh")
    r.refit_mesh(prim, pos1)
    _exact(_gpu(r, cam, opt), want2, "positions of an arena mesh: the normals are kept")
    r.refit_mesh(prim, pos0, nrm0)
    out, rad = _gpu(r, cam, gopt, 0, int(g["passes"]))
    r.close()
    assert np.array_equal(rad, g["radiance"]) and np.array_equal(out, g["accum"])


def test_refitted_normals_reach_the_feature_and_first_hit_kernels():
    """Those kernels are pinned to the reference elsewhere (tests/test_gpu_features.py, tests/test_gpu_ray_query.py); here: do they see
    the refit?  Against a fresh renderer created from the refitted pack's bytes, bit for bit."""
    import tinsel_amd
    name = "ajax_standin_96"
    scene, cam, gopt, g = _load(name)
    opt = _small(gopt)
    original = _golden_pack(name)
    prim = _mesh_prim(scene)
    pos0, nrm0 = _mesh_views(bytearray(original), prim)[0].copy(), rh.mesh_normals(bytearray(original), prim).copy()
    pos1, nrm1 = _displace(pos0, 0.05), _new_normals(nrm0, 1)
    blob = _refitted(original, prim, pos1, nrm1)
    # teeth, on the oracle: its eNormals frame of the refitted pack is not the one with the old normals, nor the one with the old positions
    nopt = opt.copy()
    nopt.mode = abi.MODE_NORMALS
    P = oa.PortOracle()
    frames = []
    for b in (blob, _refitted(original, prim, pos1, nrm0), _refitted(original, prim, pos0, nrm1)):
        h = P.load_pack(bytes(b))
        frames.append(P.render_normals(h, cam, nopt))
        P.free(h)
    assert not np.array_equal(frames[0], frames[1]) and not np.array_equal(frames[0], frames[2])

    def planes(r):
        r.init(W, H)
        f = r.features(cam, opt, 0, PASSES, which=("normal",))["normal"]
        return (f,) + tuple(r.first_hit(cam, W, H, time=0.5))

    r = tinsel_amd.create_gpu_renderer(scene)
    stale = planes(r)
    r.refit_mesh(prim, pos1, nrm1)
    got = planes(r)
    r.close()
    fresh_r = tinsel_amd.create_gpu_renderer(tinsel_amd.Scene(bytes(blob)))
    fresh = planes(fresh_r)
    fresh_r.close()
    for what, a, b, c in zip(("feature normal plane", "first-hit t", "first-hit primitive", "first-hit normal"), got, fresh, stale):
        assert a.tobytes() == b.tobytes(), "%s: %d values differ from a fresh renderer's" % (what, int((a != b).sum()))
        assert what == "first-hit primitive" or a.tobytes() != c.tobytes(), what


# -- instances ----------------------------------------------------------------------------------------------------------------------

# _displace's amount for the instanced meshes: twice as wide.  The 20 % of the tests above do not do here: every instance is turned, its leaf
# box is the box of the turned local box, and a mesh inside the unit ball that grows by 20 % along its own x stays inside most of them --
# at 96 x 72 x 2 paths the oracle renders the SAME image with the stale leaves (0 paths differ; 13 at 40 %).  At 100 % the stale leaves
# change 190 paths of mesh A's and 1,027 of mesh B's, and all but 4 of the former with only the named instance's leaf refitted.
INSTANCE_AMOUNT = 0.25


@functools.lru_cache(None)
def _instances():
    """mesh:instances:1 -- 16 primitives of 2 meshes (6 of a closed mesh of 3,504 triangles, 10 of a soup of 1,692), every third one
    moving and turning during the shutter -- with the 10-instance mesh A displaced, then the other mesh B as well; the oracle's images
    of both, computed once, and the teeth"""
    from types import SimpleNamespace
    from tests.test_gpu_mesh_scenes import made
    m = made("instances", 1)
    cam, opt, accum0, rad0 = m.frame(W, H)
    first = m.first_pass
    B, A = sorted({tuple(rh.instances(m.pack, p)) for p in rh.mesh_prims(m.pack)}, key=len)
    assert (len(B), len(A)) == (6, 10)
    moving = lambda p: bytes(rh.transforms(m.pack, p)[0]) != bytes(rh.transforms(m.pack, p)[1])
    assert any(moving(p) for p in A) and not all(moving(p) for p in A)
    prim_a, prim_b = A[1], B[-1]                                    # the mesh is named through an instance that is not its first
    pos_a0, pos_b0 = _mesh_views(bytearray(m.pack), prim_a)[0].copy(), _mesh_views(bytearray(m.pack), prim_b)[0].copy()
    pos_a1, pos_b1 = _displace(pos_a0, INSTANCE_AMOUNT), _displace(pos_b0, INSTANCE_AMOUNT)
    blob_a = _refitted(m.pack, prim_a, pos_a1)
    blob_ab = _refitted(blob_a, prim_b, pos_b1)
    before = (accum0, rad0)
    want_a, want_ab = _oracle(blob_a, cam, opt, first), _oracle(blob_ab, cam, opt, first)
    assert _differ(want_a, before) and _differ(want_ab, want_a)
    # stale leaves clip: all of them stale, and with only the named instance's leaf refitted
    stale = _refitted(m.pack, prim_a, pos_a1, scene_level=False)
    assert _differ(want_a, _oracle(stale, cam, opt, first))
    rh.refit_scene_level(stale, [prim_a])
    assert _differ(want_a, _oracle(stale, cam, opt, first))
    return SimpleNamespace(m=m, cam=cam, opt=opt, first=first, A=A, B=B, prim_a=prim_a, prim_b=prim_b, pos_a0=pos_a0, pos_b0=pos_b0,
                           pos_a1=pos_a1, pos_b1=pos_b1, blob_a=bytes(blob_a), blob_ab=bytes(blob_ab), before=before, want_a=want_a, want_ab=want_ab)


@needs_ref
def test_refit_of_an_instanced_mesh_under_every_pipeline():
    import tinsel_amd
    c = _instances()
    r = tinsel_amd.create_gpu_renderer(tinsel_amd.Scene(c.m.pack))
    r.refit_mesh(c.prim_a, c.pos_a1)
    for pipe, what in ((AUTO, "auto"), (SPLIT, "split"), (PAIRED, "paired")):
        r.set_pipeline(pipe)
        _exact(_gpu(r, c.cam, c.opt, c.first), c.want_a, "10 instances refitted, pipeline " + what)
    r.refit_mesh(c.prim_b, c.pos_b1)                                # mesh A, then mesh B
    for pipe, what in ((AUTO, "auto"), (PAIRED, "paired")):
        r.set_pipeline(pipe)
        _exact(_gpu(r, c.cam, c.opt, c.first), c.want_ab, "both meshes refitted, pipeline " + what)
    r.refit_mesh(c.prim_a, c.pos_a0)
    r.refit_mesh(c.prim_b, c.pos_b0)
    r.set_pipeline(AUTO)
    _exact(_gpu(r, c.cam, c.opt, c.first), c.before, "both meshes refitted back")
    r.close()


@needs_ref
def test_refit_of_an_instanced_mesh_under_device_built_trees():
    import tinsel_amd
    c = _instances()
    r = tinsel_amd.create_gpu_renderer(tinsel_amd.Scene(c.m.pack))
    r.refit_mesh(c.prim_a, c.pos_a1)
    r.set_mesh_bvh(abi.BVH_LBVH)                                    # built AFTER the refit: from the moved triangle records
    _device_tree_bars(_gpu(r, c.cam, c.opt, c.first), c.want_a, "instances, LBVH built after the refit")
    r.set_mesh_bvh(abi.BVH_PLOC)
    _device_tree_bars(_gpu(r, c.cam, c.opt, c.first), c.want_a, "instances, PLOC built after the refit")
    r.refit_mesh(c.prim_b, c.pos_b1)                                # refitted UNDER the device-built trees
    _device_tree_bars(_gpu(r, c.cam, c.opt, c.first), c.want_ab, "instances, PLOC trees refitted")
    r.set_mesh_bvh(abi.BVH_REFERENCE)                               # the reference's trees followed both refits
    _exact(_gpu(r, c.cam, c.opt, c.first), c.want_ab, "back on the reference trees")
    r.set_mesh_bvh(abi.BVH_LBVH)
    r.refit_mesh(c.prim_a, c.pos_a0)
    r.refit_mesh(c.prim_b, c.pos_b0)
    _device_tree_bars(_gpu(r, c.cam, c.opt, c.first), c.before, "instances, LBVH trees refitted back")
    r.set_mesh_bvh(abi.BVH_REFERENCE)
    _exact(_gpu(r, c.cam, c.opt, c.first), c.before, "refitted back under LBVH, rendered on the reference trees")
    r.close()


# -- a mesh light of thousands of triangles -------------------------------------------------------------------------------------------

@needs_ref
def test_refit_of_a_large_mesh_light_with_zero_area_triangles():
    """mesh:mesh_light:1 -- the emitter is a closed mesh of 3,128 triangles (a CDF search per light sample).  Stretched unevenly, 30 % of
    its triangles collapsed to their first vertex: zero-area steps in the CDF, a new area in the light pdf.  Then a non-emitting mesh
    with EVERY triangle collapsed: nothing of it is hit.  (A fully collapsed emitter is left out: area 0 makes the reference's own CDF NaN.)"""
    import tinsel_amd
    from tests.test_gpu_mesh_scenes import made
    m = made("mesh_light", 1)
    cam, opt, accum0, rad0 = m.frame(W, H)
    before = (accum0, rad0)
    meshes = rh.mesh_prims(m.pack)
    light = [p for p in meshes if rh.light_samples(m.pack, p) > 0]
    assert len(light) == 1
    light = light[0]
    pos0, idx = (v.copy() for v in _mesh_views(bytearray(m.pack), light)[:2])
    assert len(idx) >= 2000
    pos1 = (pos0*np.array([1.3, 0.8, 1.1], np.float32)).astype(np.float32)
    gone = np.random.default_rng(11).random(len(idx)) < 0.3
    pos1[idx[gone].ravel()] = np.repeat(pos1[idx[gone, 0]], 3, axis=0)
    blob1 = _refitted(m.pack, light, pos1)
    cdf = _mesh_views(blob1, light)[3]
    flat_steps = int((np.diff(cdf) == 0).sum())
    print("emitter: %d triangles, %d zero-area steps in the CDF" % (len(idx), flat_steps))
    assert flat_steps >= 0.25*len(idx)
    want1 = _oracle(blob1, cam, opt, m.first_pass)
    assert _differ(want1, before) and _differ(want1, _oracle(_refitted(m.pack, light, pos1, scene_level=False), cam, opt, m.first_pass))
    # the CDF and the area shade: the new vertices with the old CDF and area are another image
    old = bytearray(blob1)
    _mesh_views(old, light)[3][:] = _mesh_views(bytearray(m.pack), light)[3]
    old[_mesh_views(old, light)[4]:_mesh_views(old, light)[4] + 4] = m.pack[_mesh_views(old, light)[4]:_mesh_views(old, light)[4] + 4]
    assert _differ(want1, _oracle(old, cam, opt, m.first_pass))
    # a non-emitting soup (no shared vertices), every triangle collapsed to its first vertex
    soup = [p for p in meshes if p != light and np.array_equal(_mesh_views(bytearray(m.pack), p)[1].ravel(), np.arange(_mesh_views(bytearray(m.pack), p)[1].size))]
    assert soup
    soup = soup[0]
    spos, sidx = (v.copy() for v in _mesh_views(bytearray(m.pack), soup)[:2])
    spos1 = np.repeat(spos[sidx[:, 0]], 3, axis=0)
    assert spos1.shape == spos.shape and (spos1[sidx[:, 0]] == spos1[sidx[:, 1]]).all() and (spos1[sidx[:, 0]] == spos1[sidx[:, 2]]).all()
    blob2 = _refitted(blob1, soup, spos1)
    want2 = _oracle(blob2, cam, opt, m.first_pass)
    assert _differ(want2, want1)

    r = tinsel_amd.create_gpu_renderer(tinsel_amd.Scene(m.pack))
    r.refit_mesh(light, pos1)
    _exact(_gpu(r, cam, opt, m.first_pass), want1, "the mesh light stretched, 30 % of its triangles collapsed")
    r.refit_mesh(soup, spos1)
    _exact(_gpu(r, cam, opt, m.first_pass), want2, "a mesh with every triangle collapsed")
    r.set_pipeline(PAIRED)
    _exact(_gpu(r, cam, opt, m.first_pass), want2, "the same under the paired pipeline")
    r.close()


# -- order of operations ---------------------------------------------------------------------------------------------------------------

class _TreeOf:
    """what tests/test_gpu_bvh_build.py::check_against_host asks of a mesh: the renderer, the tree in force, the triangles it is over"""
    def __init__(self, r, prim, tris):
        self.r, self.prim, self.tris = r, prim, np.ascontiguousarray(tris, np.float32)

    def tree(self):
        return self.r.mesh_tree(self.prim)


@needs_ref
def test_a_device_build_after_a_refit_reads_the_moved_triangles():
    import tinsel_amd
    from tests.test_gpu_bvh_build import check_against_host
    c = _instances()
    r = tinsel_amd.create_gpu_renderer(tinsel_amd.Scene(c.m.pack), 0, abi.Tuning(small_mesh_bytes=0))
    idx = _mesh_views(bytearray(c.m.pack), c.prim_a)[1]
    r.refit_mesh(c.prim_a, c.pos_a1)
    for mode, label in ((abi.BVH_LBVH, "lbvh"), (abi.BVH_PLOC, "ploc")):
        r.set_mesh_bvh(mode)
        for p in (c.prim_a, c.A[0]):                                # every instance walks the one tree
            check_against_host(_TreeOf(r, p, c.pos_a1[idx]), mode, "%s after a refit, primitive %d" % (label, p))
    r.set_mesh_bvh(abi.BVH_REFERENCE)
    _exact(_gpu(r, c.cam, c.opt, c.first), c.want_a, "back on the reference trees")
    r.close()


@needs_ref
def test_two_refits_in_a_row():
    import tinsel_amd
    c = _instances()
    first = _displace(c.pos_a0, 0.1)
    assert _differ(_oracle(_refitted(c.m.pack, c.prim_a, first), c.cam, c.opt, c.first), c.want_a)
    r = tinsel_amd.create_gpu_renderer(tinsel_amd.Scene(c.m.pack))
    r.refit_mesh(c.A[0], first)                                     # no render in between
    r.refit_mesh(c.prim_a, c.pos_a1)
    _exact(_gpu(r, c.cam, c.opt, c.first), c.want_a, "the second of two refits")
    r.close()


@needs_ref
def test_move_rebuild_then_refit():
    """set_primitive_transform + rebuild_scene, THEN refit_mesh: the leaf boxes and PrimitiveArea (area * endTransform.s, the light pdf)
    of the refit must come from the new transforms.  One static instance of mesh A is made an emitter in the pack (the material and
    light samples of the scene's sphere light), moved and scaled by 1.5; another static one is made to move during the shutter; the mesh
    is refitted through a third."""
    import ctypes
    import tinsel_amd
    c = _instances()
    static = [p for p in c.A if p != c.prim_a and bytes(rh.transforms(c.m.pack, p)[0]) == bytes(rh.transforms(c.m.pack, p)[1])]
    emitter, mover = static[0], static[1]
    lamp = [p for p in range(rh.num_primitives(c.m.pack)) if rh.light_samples(c.m.pack, p) > 0][-1]
    base = bytearray(c.m.pack)
    for off, n in ((rh.OFF_MATERIAL, ctypes.sizeof(abi.Material)), (rh.OFF_LIGHT_SAMPLES, 4)):
        src, dst = rh.prim_base(base, lamp) + off, rh.prim_base(base, emitter) + off
        base[dst:dst + n] = base[src:src + n]
    base = bytes(base)

    copy = lambda t: abi.Transform.from_buffer_copy(bytes(t))
    e_start = copy(rh.transforms(base, emitter)[0])
    e_start.p.x += 0.4
    e_start.p.y += 0.3
    e_start.s *= 1.5
    m_start = copy(rh.transforms(base, mover)[0])
    m_end = copy(m_start)
    m_end.p.y += 0.5
    m_end.p.z += 0.25
    moved = bytearray(base)
    rh.set_transform(moved, emitter, e_start)
    rh.set_transform(moved, mover, m_start, m_end)
    stale = _refitted(moved, c.prim_a, c.pos_a1, scene_level=False)            # leaves of the old transforms and the old mesh
    _refit_pack(moved, c.prim_a, c.pos_a0)                                     # the new transforms, the mesh as it was
    nodes = rh.scene_nodes(moved)
    final = _refitted(moved, c.prim_a, c.pos_a1)
    want = _oracle(final, c.cam, c.opt, c.first)
    assert _differ(want, _oracle(base, c.cam, c.opt, c.first)) and _differ(want, _oracle(moved, c.cam, c.opt, c.first))
    assert _differ(want, _oracle(stale, c.cam, c.opt, c.first))
    # ... and the emitter's area shades: with the area of the mesh as it was in that one instance's record the oracle gives another image
    old_area = bytearray(final)
    at = rh.prim_base(old_area, emitter) + rh.OFF_AREA
    old_area[at:at + 4] = base[at:at + 4]
    assert _differ(want, _oracle(old_area, c.cam, c.opt, c.first))

    r = tinsel_amd.create_gpu_renderer(tinsel_amd.Scene(base))
    r.set_primitive_transform(emitter, e_start)
    r.set_primitive_transform(mover, m_start, m_end)
    r.rebuild_scene(nodes)
    r.refit_mesh(c.prim_a, c.pos_a1)
    for pipe, what in ((AUTO, "auto"), (SPLIT, "split")):
        r.set_pipeline(pipe)
        _exact(_gpu(r, c.cam, c.opt, c.first), want, "moved, rebuilt, refitted, pipeline " + what)
    r.close()


@needs_ref
def test_refit_then_a_device_rebuild_of_the_scene_level():
    """rebuild_scene() on the device after a refit: its leaf boxes are PrimitiveBounds of the mesh roots as the refit left them"""
    import tinsel_amd
    c = _instances()
    r = tinsel_amd.create_gpu_renderer(tinsel_amd.Scene(c.m.pack))
    r.refit_mesh(c.prim_a, c.pos_a1)
    r.rebuild_scene()
    _device_tree_bars(_gpu(r, c.cam, c.opt, c.first), c.want_a, "scene level rebuilt on the device after a refit")
    r.rebuild_scene(rh.scene_nodes(c.blob_a))
    _exact(_gpu(r, c.cam, c.opt, c.first), c.want_a, "the refitted pack's own scene tree afterwards")
    r.close()


# -- a ray query ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not oa.have_ref_trace(), reason="oracle/_ref not built, or without ref_leaf_trace")
def test_ray_queries_follow_the_refitted_instances():
    """closest-hit trace_rays on mesh:instances:1 after the refit against the reference's Trace() on the refitted pack: hit, t, primitive
    and normal bit for bit, every ray (rays and the per-primitive check: tests/test_gpu_ray_query.py's own)"""
    import tinsel_amd
    from tests.test_gpu_ray_query import _check_closest, _rays
    c = _instances()
    R = _ref()
    h = R.load_pack(c.blob_a)
    rays = _rays(R, h, 20261019)
    rows = np.ascontiguousarray(rays[:, [0, 1, 2, 4, 5, 6, 3]])
    wp, wt, wn = R.trace(h, rows)
    for other in (c.m.pack, bytes(_refitted(c.m.pack, c.prim_a, c.pos_a1, scene_level=False))):      # teeth: before, and with stale leaves
        h2 = R.load_pack(other)
        op, ot, _ = R.trace(h2, rows)
        R.free(h2)
        assert not np.array_equal(op, wp) and not np.array_equal(ot.view(np.uint32), wt.view(np.uint32))
    r = tinsel_amd.create_gpu_renderer(tinsel_amd.Scene(c.m.pack))
    r.refit_mesh(c.prim_a, c.pos_a1)
    rec = r.trace_rays(rays, "closest")
    r.close()
    try:
        _check_closest(R, h, "mesh:instances:1 refitted", rays, rec)
    finally:
        R.free(h)
    got_n = np.stack([rec["nx"], rec["ny"], rec["nz"]], axis=1)
    differ = (int(((rec["primitive"] >= 0) != (wp >= 0)).sum()), int((rec["primitive"] != wp).sum()),
              int((rec["t"].view(np.uint32) != wt.view(np.uint32)).sum()), int((got_n.view(np.uint32) != wn.view(np.uint32)).any(axis=1).sum()))
    assert differ == (0, 0, 0, 0), "rays that differ from Trace() in (hit, primitive, t, normal): %s" % (differ,)

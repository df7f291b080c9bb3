"""Baked instances (tn_baked.h, tn_host_bake.h): the closed FIT kernel compiled for one scene's wave-uniform level, against the library's own
instance -- the bake mode (abi.Tuning bounce_bake, tinsel_hip_set_bounce_bake) 1 against 0 on the SAME renderer, bit for bit on the
accumulator and the per-path radiance (`batch_radiance`), with tinsel_hip_bake_status saying which function served the launches; against
the golden and, where oracle/_ref is built, the live reference. The module's compiles share one cache directory, so a scene is compiled
once."""
import ctypes as C
import os

import numpy as np
import pytest

import tinsel_amd
from tinsel_amd import abi, create_gpu_renderer
from tinsel_amd import build as hb
from tests import oracle_api as oa

pytestmark = pytest.mark.gpu

F = abi
INSTALLED = (F.BAKE_COMPILED, F.BAKE_FROM_CACHE)


@pytest.fixture(scope="module", autouse=True)
def bake_cache(tmp_path_factory):
    was = os.environ.get(hb.BAKE_CACHE_ENV)
    os.environ[hb.BAKE_CACHE_ENV] = str(tmp_path_factory.mktemp("bake_cache"))
    yield os.environ[hb.BAKE_CACHE_ENV]
    if was is None:
        del os.environ[hb.BAKE_CACHE_ENV]
    else:
        os.environ[hb.BAKE_CACHE_ENV] = was


def _golden(name):
    g = np.load(os.path.join(oa.GOLDEN, name + ".golden.npz"))
    return g, abi.Camera.from_buffer_copy(g["camera"].tobytes()), abi.Options.from_buffer_copy(g["options"].tobytes())


def _pack_bytes(name):
    with open(os.path.join(oa.GOLDEN, name + ".pack"), "rb") as fh:
        return fh.read()


def _prims(scene):
    return (abi.Primitive*scene.num_primitives).from_address(scene.desc.primitives)


def _edit_planes(name, edits):
    """the pack's bytes with plane equations rewritten ({equation: new equation}), the way tests/test_gpu_plane_pairs.py edits scenes"""
    raw = bytearray(_pack_bytes(name))
    scene = tinsel_amd.Scene(bytes(raw))
    prims = _prims(scene)
    for eq, new in edits.items():
        k = next(i for i, p in enumerate(prims) if p.type == abi.GEOM_PLANE and tuple(p.geo.plane.plane) == tuple(np.float32(v) for v in eq))
        off = C.addressof(prims[k].geo.plane) - C.addressof(scene._buf)
        raw[off:off + 16] = np.asarray(new, np.float32).tobytes()
    return bytes(raw)


def _render(r, cam, opt, passes):
    r.init(opt.width, opt.height)
    r.set_pass_index(0)
    out = r.render(cam, opt, passes=passes)
    return out, r.batch_radiance(passes, opt.height, opt.width)


def _both(r, cam, opt, passes, served=True):
    """((accumulator, radiance) baked, the same with bounce_bake = 0) on one renderer; `served`: must the baked function have run?"""
    r.set_tuning(bounce_bake=1)
    st = r.bake()
    assert st["state"] in INSTALLED, st
    before = st["launches"]
    on = _render(r, cam, opt, passes)
    after = r.bake_status()
    assert (after["launches"] > before) == served, (before, after)
    assert not served or r.bounce_plan()[0] == F.BOUNCE_FIT_CLOSED      # (the plan keeps reporting the closed kind and its features)
    r.set_tuning(bounce_bake=0)
    assert r.bake_status()["state"] == F.BAKE_OFF
    off = _render(r, cam, opt, passes)
    assert r.bake_status()["launches"] == after["launches"]
    r.set_tuning(bounce_bake=1)
    return on, off


def _assert_same(a, b, lit=True):
    assert np.isfinite(a[0]).all() and (a[0][..., :3].any() or not lit)
    assert np.array_equal(a[1], b[1]), "%d paths differ" % int((a[1] != b[1]).any(axis=-1).sum())
    assert np.array_equal(a[0], b[0])


def _reference(pack, cam, opt, passes):
    if not oa.have_ref():
        return None
    R = oa.RefOracle()
    h = R.load_pack(pack)
    accum, rad, _ = R.render_seeded(h, cam, opt, 0, passes, want_accum=True, want_radiance=True)
    R.free(h)
    return accum, rad


def _small(opt, depth=None):
    o = opt.copy()
    o.width, o.height = 64, 48
    if depth is not None:
        o.max_depth = depth
    return o


@pytest.mark.parametrize("depth", [1, 4, 7])
def test_cornell_small_frames(depth):
    scene = tinsel_amd.Scene(_pack_bytes("cornell"))
    _, cam, opt = _golden("cornell")
    r = create_gpu_renderer(scene, 0, abi.Tuning(bounce_share=0))
    on, off = _both(r, cam, _small(opt, depth), 3)
    r.close()
    _assert_same(on, off)


def test_cornell_at_the_plans_own_cut():
    """1024 x 1024 x 3 in one batch with the default tuning: the regions the headline runs with"""
    scene = tinsel_amd.Scene(_pack_bytes("cornell"))
    _, cam, opt = _golden("cornell")
    o = opt.copy()
    o.width, o.height = 1024, 1024
    r = create_gpu_renderer(scene)
    on, off = _both(r, cam, o, 3)
    r.close()
    _assert_same(on, off)


def test_cornells_golden_and_the_live_reference():
    scene = tinsel_amd.Scene(_pack_bytes("cornell"))
    g, cam, opt = _golden("cornell")
    passes = int(g["passes"])
    r = create_gpu_renderer(scene, 0, abi.Tuning(bounce_share=0))
    on, off = _both(r, cam, opt, passes)
    r.close()
    _assert_same(on, off)
    assert np.array_equal(on[1], g["radiance"]) and np.array_equal(on[0], g["accum"])
    ref = _reference(_pack_bytes("cornell"), cam, opt, passes)
    if ref is not None:
        assert np.array_equal(on[1], ref[1]) and np.array_equal(on[0], ref[0])


def test_a_one_pixel_frame():
    """the pixel's rays run along the view axis: zero denominators in both pairs, pose_rotate's zero-component branches"""
    scene = tinsel_amd.Scene(_pack_bytes("cornell"))
    _, cam, opt = _golden("cornell")
    o = opt.copy()
    o.width, o.height = 1, 1
    r = create_gpu_renderer(scene, 0, abi.Tuning(bounce_share=0))
    on, off = _both(r, cam, o, 16)
    r.close()
    _assert_same(on, off)
    ref = _reference(_pack_bytes("cornell"), cam, o, 16)
    if ref is not None:
        assert np.array_equal(on[1], ref[1]) and np.array_equal(on[0], ref[0])


# (equations rewritten, the tuning's plane_pairs, the plane table that results)
EDITS = {
    "camera-above-the-ceiling": ({}, -1, (2, 1)),
    "one-wall-scaled-by-2": ({(1.0, 0.0, 0.0, 1.0): (2.0, 0.0, 0.0, 2.0)}, -1, (1, 3)),
    "single-planes-only": ({}, 0, (0, 5)),
}


@pytest.mark.parametrize("edit", list(EDITS))
def test_edited_cornells_from_above_the_ceiling(edit):
    """The camera above the ceiling: a primary ray that points down has the floor AND the ceiling ahead, so its wave leaves the pair block and
    takes the table slot by slot (the run-time fallback a baked instance keeps); one pair dissolved into two singles; no pairs at all."""
    edits, pairs, table = EDITS[edit]
    pack = _edit_planes("cornell", edits)
    scene = tinsel_amd.Scene(pack)
    _, cam, opt = _golden("cornell")
    cam = abi.Camera.from_buffer_copy(bytes(cam))
    cam.position.y = 2.5
    o = opt.copy()
    o.width, o.height = 96, 64
    r = create_gpu_renderer(scene, 0, abi.Tuning(bounce_share=0, plane_pairs=pairs))
    assert r.plane_table() == table
    on, off = _both(r, cam, o, 3)
    r.close()
    # (from up there nearly every path is black -- what it reaches lies above the ceiling plane, which hides the lamp from all but the points
    # right above it, and a small frame may have none -- so a lit pixel is not asked for: what is compared is every path's radiance and
    # the filter weights, with the library's instance and with the live reference)
    _assert_same(on, off, lit=False)
    assert on[0][..., 3].any()
    ref = _reference(pack, cam, o, 3)
    if ref is not None:
        assert np.array_equal(on[1], ref[1]) and np.array_equal(on[0], ref[0])


def _spheres_as_planes(name, eqs):
    """the pack with its first len(eqs) spheres turned into planes, each one's leaf of the scene BVH made the "infinite" box a plane has (so
    that create puts it into the plane table); the internal nodes above those leaves are stale until rebuild_scene()"""
    raw = bytearray(_pack_bytes(name))
    scene = tinsel_amd.Scene(bytes(raw))
    prims, base, d = _prims(scene), C.addressof(scene._buf), scene.desc
    nodes = (abi.BVHNode*d.num_bvh_nodes).from_address(C.cast(d.bvh_nodes, C.c_void_p).value)
    spheres = [i for i, p in enumerate(prims) if p.type == abi.GEOM_SPHERE]
    for k, eq in zip(spheres, eqs):
        off = C.addressof(prims[k]) - base + abi.Primitive.type.offset
        raw[off:off + 4] = np.int32(abi.GEOM_PLANE).tobytes()
        off = C.addressof(prims[k].geo.plane) - base
        raw[off:off + 16] = np.asarray(eq, np.float32).tobytes()
        for n in nodes:
            if (n.right_index_leaf >> 31) and n.left_index == k:
                off = C.addressof(n) - base
                raw[off:off + 24] = np.asarray([-1e8]*3 + [1e8]*3, np.float32).tobytes()
    return bytes(raw)


# (spheres turned into planes, planes shrunk out of the table, the plane table that results, does a sphere remain)
MIXES = {
    # a wall far behind the camera closes the box: with the back wall a third pair -- two blocks, the second read by the blocks of four
    "six-planes-three-pairs": ([(0.0, 0.0, -1.0, 50.0)], [], (3, 0), True),
    # both spheres gone: the scan visits the lamp only, no sphere code is asked for
    "no-sphere": ([(0.0, 0.0, -1.0, 50.0), (0.0, 0.0, -1.0, 60.0)], [], (3, 1), False),
    # the ceiling and a wall scaled out of the table: their partners and the back wall are three single planes, no pair block
    "three-single-planes": ([], [(0.0, -1.0, 0.0, 2.0), (1.0, 0.0, 0.0, 1.0)], (0, 3), True),
}


@pytest.mark.parametrize("mix", list(MIXES))
def test_other_mixes_of_primitives(mix):
    to_planes, shrunk, table, sphere = MIXES[mix]
    scene = tinsel_amd.Scene(_spheres_as_planes("cornell", to_planes))
    prims = _prims(scene)
    assert any(p.type == abi.GEOM_SPHERE for p in prims) == sphere
    _, cam, opt = _golden("cornell")
    r = create_gpu_renderer(scene, 0, abi.Tuning(bounce_share=0))
    for eq in shrunk:
        k = next(i for i, p in enumerate(prims) if p.type == abi.GEOM_PLANE and tuple(p.geo.plane.plane) == tuple(np.float32(v) for v in eq))
        small = abi.Transform.from_buffer_copy(bytes(prims[k].start_transform))
        small.s = 2e-8                      # PrimitiveBounds: +-1e8 times the scale -- a bounded leaf box, so the plane leaves the table
        r.set_primitive_transform(k, small, small)
    r.rebuild_scene()
    assert r.plane_table() == table
    assert bool(r.bake_source()[0]) and r.bake_source()[2]
    on, off = _both(r, cam, _small(opt), 3)
    r.close()
    _assert_same(on, off)


def test_shared_regions_run_the_general_kernel():
    """64 x 48 with the default sharing: the plan picks the general kernel, the installed function serves nothing, the image is the same"""
    scene = tinsel_amd.Scene(_pack_bytes("cornell"))
    _, cam, opt = _golden("cornell")
    r = create_gpu_renderer(scene)
    on, off = _both(r, cam, _small(opt), 3, served=False)
    assert r.bounce_plan()[0] == F.BOUNCE_GENERAL
    r.close()
    _assert_same(on, off)


def test_mode_1_bakes_at_the_first_render_without_a_reserve():
    """no reserve(), no bake(): the first render under mode 1 compiles (or finds) and installs, and is served; switching the mode alone keeps
    the path buffers (nothing of the C tuning changes)"""
    scene = tinsel_amd.Scene(_pack_bytes("cornell"))
    _, cam, opt = _golden("cornell")
    r = create_gpu_renderer(scene, 0, abi.Tuning(bounce_share=0, bounce_bake=1))
    assert r.bake_status()["state"] == F.BAKE_NONE
    on = _render(r, cam, _small(opt), 3)
    st = r.bake_status()
    assert st["state"] in INSTALLED and st["launches"] > 0
    r.set_tuning(bounce_bake=0)
    assert r.get_tuning().bounce_bake == 0 and r.get_tuning().bounce_share == 0 and r.bake_status()["state"] == F.BAKE_OFF
    off = _render(r, cam, _small(opt), 3)
    assert r.bake_status()["launches"] == st["launches"]
    r.close()
    _assert_same(on, off)


def test_the_tolerance_arm_is_never_served():
    scene = tinsel_amd.Scene(_pack_bytes("cornell"))
    _, cam, opt = _golden("cornell")
    r = create_gpu_renderer(scene, 0, abi.Tuning(bounce_share=0, bounce_bake=1))
    assert r.bake()["state"] in INSTALLED
    r.set_arithmetic(abi.ARITH_FAST)
    out, _ = _render(r, cam, _small(opt), 3)
    assert r.bake_status()["launches"] == 0 and np.isfinite(out).all()
    r.close()


def _move_a_sphere(r, scene):
    prims = _prims(scene)
    k = next(i for i, p in enumerate(prims) if p.type == abi.GEOM_SPHERE)
    t = abi.Transform.from_buffer_copy(bytes(prims[k].start_transform))
    t.p.x += 0.125
    r.set_primitive_transform(k, t, t)
    r.rebuild_scene()


def test_a_moved_sphere_makes_the_module_stale_until_the_next_reserve():
    scene = tinsel_amd.Scene(_pack_bytes("cornell"))
    _, cam, opt = _golden("cornell")
    o = _small(opt)
    r = create_gpu_renderer(scene, 0, abi.Tuning(bounce_share=0, bounce_bake=1))
    r.init(o.width, o.height)
    r.reserve(3, o.max_depth)
    first = r.bake_status()
    assert first["state"] in INSTALLED
    _move_a_sphere(r, scene)
    stale = r.bake_status()
    assert stale["state"] == F.BAKE_STALE and stale["key"] == first["key"] != r.bake_source()[1]
    # (mode 1 would bake again at the next render, tested above: the auto mode bakes at a large reserve() only, so under it a render
    # finds the stale module, which must not serve)
    r.set_tuning(bounce_bake=-1)
    moved = _render(r, cam, o, 3)
    assert r.bake_status() == stale and stale["launches"] == 0
    r.set_tuning(bounce_bake=1)

    fresh = create_gpu_renderer(tinsel_amd.Scene(_pack_bytes("cornell")), 0, abi.Tuning(bounce_share=0, bounce_bake=0))
    _move_a_sphere(fresh, scene)
    want = _render(fresh, cam, o, 3)
    fresh.close()
    _assert_same(moved, want)

    r.reserve(3, o.max_depth)
    again = r.bake_status()
    assert again["state"] in INSTALLED and again["key"] == r.bake_source()[1] != first["key"]
    baked = _render(r, cam, o, 3)
    assert r.bake_status()["launches"] > 0
    r.close()
    _assert_same(baked, want)


def test_a_second_renderer_installs_from_the_cache(bake_cache):
    scene = tinsel_amd.Scene(_pack_bytes("cornell"))
    _, cam, opt = _golden("cornell")
    a = create_gpu_renderer(scene, 0, abi.Tuning(bounce_share=0, bounce_bake=1))
    assert a.bake()["state"] in INSTALLED
    files = sorted(os.listdir(bake_cache))
    b = create_gpu_renderer(scene, 0, abi.Tuning(bounce_share=0, bounce_bake=1))
    st = b.bake()
    assert st["state"] == F.BAKE_FROM_CACHE and st["key"] == a.bake_status()["key"] == scene.bake_source()[1]
    assert sorted(os.listdir(bake_cache)) == files
    # (the description's twin and the live one agree on the text, too)
    assert b.bake_source()[:3] == scene.bake_source(abi.Tuning(bounce_share=0, bounce_bake=1))[:3]
    ra, rb = _render(a, cam, _small(opt), 3), _render(b, cam, _small(opt), 3)
    assert a.bake_status()["launches"] > 0 and b.bake_status()["launches"] > 0
    a.close()
    b.close()
    _assert_same(ra, rb)

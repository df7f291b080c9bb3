"""Opposing plane pairs in the flat scan (trace_flat, tn_plane.h): every render with the pairs against tinsel_hip_tuning::plane_pairs = 0
-- the plane table as single planes, the IntersectRayPlane calls as they were -- on the SAME renderer, bit for bit on the accumulator and
the per-path radiance; against the golden where a fixture exists, and against the live reference (oracle/_ref) for the edited scenes
where it is built."""
import ctypes as C
import os

import numpy as np
import pytest

import tinsel_amd
from tinsel_amd import abi, create_gpu_renderer
from tests import oracle_api as oa

pytestmark = pytest.mark.gpu

F = abi


def _golden(name):
    g = np.load(os.path.join(oa.GOLDEN, name + ".golden.npz"))
    return g, abi.Camera.from_buffer_copy(g["camera"].tobytes()), abi.Options.from_buffer_copy(g["options"].tobytes())


def _pack_bytes(name):
    with open(os.path.join(oa.GOLDEN, name + ".pack"), "rb") as fh:
        return fh.read()


def _planes(scene):
    prims = (abi.Primitive*scene.num_primitives).from_address(scene.desc.primitives)
    return prims, [i for i, p in enumerate(prims) if p.type == abi.GEOM_PLANE]


def _plane_with(scene, eq):
    prims, planes = _planes(scene)
    return next(i for i in planes if tuple(prims[i].geo.plane.plane) == tuple(np.float32(v) for v in eq))


def _edit_pack(name, edits):
    """the pack's bytes with plane equations rewritten ({equation: new equation}): an opened pack is relocated in place, so the offsets are
    taken from an opened copy and the edit is made in the file's own bytes -- which the reference loads too"""
    raw = bytearray(_pack_bytes(name))
    scene = tinsel_amd.Scene(bytes(raw))
    prims, _ = _planes(scene)
    for eq, new in edits.items():
        k = _plane_with(scene, eq)
        off = C.addressof(prims[k].geo.plane) - C.addressof(scene._buf)
        assert np.frombuffer(raw, np.float32, 4, off).tolist() == list(eq)
        raw[off:off + 16] = np.asarray(new, np.float32).tobytes()
    return bytes(raw)


def _both(r, cam, opt, passes, radiance=True):
    """((accumulator, radiance) with the pairs, the same with plane_pairs = 0, the plane tables) on one renderer"""
    got = []
    for pairs in (-1, 0):
        r.set_tuning(plane_pairs=pairs)
        table = r.plane_table()
        r.init(opt.width, opt.height)
        r.set_pass_index(0)
        out = r.render(cam, opt, passes=passes)
        got.append((out, r.batch_radiance(passes, opt.height, opt.width) if radiance else None, table))
    r.set_tuning(plane_pairs=-1)
    return got


def _assert_same(a, b):
    assert np.isfinite(a[0]).all() and a[0][..., :3].any()
    if a[1] is not None:
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


@pytest.mark.parametrize("depth", [1, 4, 7])
def test_the_closed_instance_on_cornell(depth):
    """512 x 512 x 12 passes in one batch: k_bounce's closed FIT instance (tests/test_gpu_slim_state.py), two pairs and the single in one block"""
    scene = tinsel_amd.Scene(_pack_bytes("cornell"))
    _, cam, opt = _golden("cornell")
    o = opt.copy()
    o.width, o.height, o.max_depth = 512, 512, depth
    r = create_gpu_renderer(scene, 0, abi.Tuning(batch_paths=1 << 22))
    on, off = _both(r, cam, o, 12)
    assert r.bounce_plan()[0] == F.BOUNCE_FIT_CLOSED
    r.close()
    assert on[2] == (2, 1) and off[2] == (0, 5)
    _assert_same(on, off)


def test_the_general_kernel_with_shared_regions_on_cornell_and_its_golden():
    scene = tinsel_amd.Scene(_pack_bytes("cornell"))
    g, cam, opt = _golden("cornell")
    r = create_gpu_renderer(scene, 0, abi.Tuning(bounce_fit=0, bounce_share=1))
    on, off = _both(r, cam, opt, int(g["passes"]))
    assert r.bounce_plan()[0] == F.BOUNCE_GENERAL
    r.close()
    assert on[2] == (2, 1)
    _assert_same(on, off)
    assert np.array_equal(on[1], g["radiance"]) and np.array_equal(on[0], g["accum"])


def test_veach_keeps_single_planes_and_its_bits():
    """200 x 152 x 3: the deferred instance carries no pair code and its scenes form no pairs -- the switch changes nothing"""
    scene = tinsel_amd.Scene(_pack_bytes("veach"))
    _, cam, opt = _golden("veach")
    o = opt.copy()
    o.width, o.height = 200, 152
    r = create_gpu_renderer(scene, 0, abi.Tuning(batch_paths=1 << 22))
    on, off = _both(r, cam, o, 3)
    r.close()
    assert on[2] == off[2] and on[2][0] == 0
    _assert_same(on, off)


def test_the_split_pipelines_scan_on_glass_and_its_golden():
    scene = tinsel_amd.Scene(_pack_bytes("glass"))
    g, cam, opt = _golden("glass")
    o = opt.copy()
    o.width, o.height, o.max_depth = 96, 64, 12
    r = create_gpu_renderer(scene)
    on, off = _both(r, cam, o, 2)
    pairs = len(scene.plane_pairs()[0])
    assert pairs >= 1 and on[2][0] == pairs and off[2][0] == 0 and sum(off[2]) == 2*pairs + on[2][1]
    _assert_same(on, off)
    gold = _both(r, cam, opt, int(g["passes"]))[0]
    r.close()
    assert np.array_equal(gold[1], g["radiance"]) and np.array_equal(gold[0], g["accum"])


@pytest.mark.parametrize("pipe", [abi.PIPELINE_AUTO, abi.PIPELINE_WAVEFRONT_SPLIT, abi.PIPELINE_MEGAKERNEL])
def test_every_pipeline_on_cornell(pipe):
    scene = tinsel_amd.Scene(_pack_bytes("cornell"))
    g, cam, opt = _golden("cornell")
    r = create_gpu_renderer(scene)
    r.set_pipeline(pipe)
    on, off = _both(r, cam, opt, int(g["passes"]))
    r.close()
    _assert_same(on, off)
    assert np.array_equal(on[1], g["radiance"]) and np.array_equal(on[0], g["accum"])


# (equations rewritten, the plane table that results)
EDITS = {
    "camera-above-the-ceiling": ({}, (2, 1)),
    # one wall of a pair scaled: no longer the other's negation -- that pair is two single planes
    "one-wall-scaled-by-2": ({(1.0, 0.0, 0.0, 1.0): (2.0, 0.0, 0.0, 2.0)}, (1, 3)),
    # both scaled, zeros of either sign: a pair whose normals are not unit
    "a-pair-scaled-by-2": ({(0.0, 1.0, 0.0, 0.0): (0.0, 2.0, -0.0, 0.0), (0.0, -1.0, 0.0, 2.0): (-0.0, -2.0, 0.0, 4.0)}, (2, 1)),
}


@pytest.mark.parametrize("edit", list(EDITS))
def test_edited_cornells_from_above_the_ceiling(edit):
    """The camera above the ceiling plane: every primary ray that points down has the floor AND the ceiling ahead, so its wave leaves the
    pairs (trace_flat's wave-uniform fallback); the paths' later rays start inside the box."""
    edits, table = EDITS[edit]
    pack = _edit_pack("cornell", edits)
    scene = tinsel_amd.Scene(pack)
    _, cam, opt = _golden("cornell")
    cam = abi.Camera.from_buffer_copy(bytes(cam))
    cam.position.y = 2.5
    o = opt.copy()
    o.width, o.height = 96, 64
    r = create_gpu_renderer(scene)
    on, off = _both(r, cam, o, 3)
    r.close()
    assert on[2] == table and off[2] == (0, 5)
    _assert_same(on, off)
    ref = _reference(pack, cam, o, 3)
    if ref is not None:
        assert np.array_equal(on[1], ref[1]) and np.array_equal(on[0], ref[0])


def test_a_one_pixel_frame():
    """the pixel's rays run along the view axis: denominators that are zeros, of either sign, in both pairs"""
    scene = tinsel_amd.Scene(_pack_bytes("cornell"))
    _, cam, opt = _golden("cornell")
    o = opt.copy()
    o.width, o.height = 1, 1
    r = create_gpu_renderer(scene)
    on, off = _both(r, cam, o, 16)
    r.close()
    _assert_same(on, off)
    ref = _reference(_pack_bytes("cornell"), cam, o, 16)
    if ref is not None:
        assert np.array_equal(on[1], ref[1]) and np.array_equal(on[0], ref[0])


def test_normals_keep_each_planes_own_zero_signs():
    """eNormals prints the hit normal: B's is B's as stored, not A's negated (cornell's `-1 0 0 1` has +0 where `1 0 0 1` negated has -0)"""
    scene = tinsel_amd.Scene(_pack_bytes("cornell"))
    g, cam, opt = _golden("cornell")
    o = opt.copy()
    o.mode = abi.MODE_NORMALS
    r = create_gpu_renderer(scene)
    on, off = _both(r, cam, o, 1, radiance=False)
    r.close()
    assert on[0].tobytes() == off[0].tobytes() and np.array_equal(on[0], g["normals"])


def test_a_pair_dissolves_and_forms_again_through_rebuild_scene():
    scene = tinsel_amd.Scene(_pack_bytes("cornell"))
    g, cam, opt = _golden("cornell")
    prims, _ = _planes(scene)
    k = _plane_with(scene, (0.0, -1.0, 0.0, 2.0))
    d = scene.desc
    nodes = (abi.BVHNode*d.num_bvh_nodes).from_buffer_copy(C.string_at(C.cast(d.bvh_nodes, C.c_void_p), d.num_bvh_nodes*C.sizeof(abi.BVHNode)))
    here = abi.Transform.from_buffer_copy(bytes(prims[k].start_transform))
    small = abi.Transform.from_buffer_copy(bytes(prims[k].start_transform))
    small.s = 2e-8                       # PrimitiveBounds: +-1e8 times the scale -- a bounded leaf box, so the plane leaves the table
    r = create_gpu_renderer(scene)
    first = _both(r, cam, opt, int(g["passes"]))
    assert first[0][2] == (2, 1)
    r.set_primitive_transform(k, small, small)
    r.rebuild_scene()
    moved = _both(r, cam, opt, int(g["passes"]))
    assert moved[0][2][0] < 2 and sum(moved[0][2]) == 4 and moved[1][2] == (0, 4)
    _assert_same(moved[0], moved[1])
    r.set_primitive_transform(k, here, here)
    r.rebuild_scene(nodes)
    back = _both(r, cam, opt, int(g["passes"]))
    r.close()
    assert back[0][2] == (2, 1) and back[1][2] == (0, 5)
    _assert_same(back[0], back[1])
    assert np.array_equal(back[0][1], g["radiance"]) and np.array_equal(back[0][0], g["accum"])

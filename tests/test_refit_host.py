"""tests/refit_host.py against the reference's own builder: a host refit with the UNCHANGED vertices and normals must leave a pack byte
for byte as the reference wrote it -- its mesh nodes (Mesh::RebuildBVH), CDF and area (Mesh::RebuildCDF), and its scene BVH
(Scene::Build over PrimitiveBounds), for every instance of every mesh: veach's rotated mesh and the moving instances of the generated
`instances` scene included.  That is what makes the refitted packs of tests/test_gpu_refit.py an oracle: the only thing the helper adds
to the reference's output is the new vertices."""
import os

import numpy as np
import pytest

from tests import oracle_api as oa
from tests import refit_host as rh

pytestmark = pytest.mark.skipif(not oa.have_port(), reason="oracle/libtinsel_oracle.so not built")

GOLDEN_PACKS = ["cornell", "ajax_standin_96", "glass", "veach"]
GENERATED = ["mesh:instances:1", "mesh:mesh_light:1", "mesh:seven:1"]


def _pack(name):
    if name.startswith("mesh:"):
        from tests.test_gpu_mesh_scenes import pack_bytes
        return pack_bytes(name)                     # (skips where oracle/_ref is absent: the reference's loader makes these)
    with open(os.path.join(oa.GOLDEN, name + ".pack"), "rb") as fh:
        return fh.read()


@pytest.mark.parametrize("name", GOLDEN_PACKS + GENERATED)
def test_a_host_refit_with_the_unchanged_mesh_leaves_the_pack_byte_for_byte(name):
    original = _pack(name)
    blob = bytearray(original)
    meshes = {}                                     # position block -> its instances
    for p in rh.mesh_prims(blob):
        meshes.setdefault(tuple(rh.instances(blob, p)), p)
    assert meshes, name
    for same_mesh, first in meshes.items():
        through = same_mesh[-1]                     # (any instance names the mesh: not the first one where there are several)
        pos = rh.mesh_views(blob, through)[0].copy()
        nrm = rh.mesh_normals(blob, through).copy()
        rh.refit_pack(blob, through, pos, nrm)
    differ = np.frombuffer(bytes(blob), np.uint8) != np.frombuffer(original, np.uint8)
    print("%s: %d meshes, %d mesh primitives, %d of %d bytes differ" % (name, len(meshes), sum(map(len, meshes)), int(differ.sum()), len(original)))
    assert not differ.any(), "%s: %d bytes differ, the first at offset %d" % (name, int(differ.sum()), int(np.argmax(differ)))


@pytest.mark.skipif(not oa.have_ref(), reason="oracle/_ref not built")
def test_the_generated_instances_scene_stores_one_block_per_mesh():
    blob = bytearray(_pack("mesh:instances:1"))
    groups = sorted({tuple(rh.instances(blob, p)) for p in rh.mesh_prims(blob)}, key=len)
    assert [len(g) for g in groups] == [6, 10], groups
    for g in groups:
        moving = [p for p in g if bytes(rh.transforms(blob, p)[0]) != bytes(rh.transforms(blob, p)[1])]
        assert moving and len(moving) < len(g), (g, moving)


def test_set_transform_and_refit_give_the_reference_leaf_of_the_moved_primitive():
    """set_transform + refit_pack(scene_level=True): moving a primitive there and back restores the pack, and in between its leaf is the
    oracle's PrimitiveBounds (itself pinned to the reference's in tests/test_oracle.py) with every ancestor the union of its children"""
    original = _pack("veach")
    blob = bytearray(original)
    prim = rh.mesh_prims(blob)[0]
    start, end = rh.transforms(blob, prim)
    moved = type(start).from_buffer_copy(bytes(start))
    moved.p.x += 0.75
    moved.s *= 1.5
    pos = rh.mesh_views(blob, prim)[0].copy()
    rh.set_transform(blob, prim, moved, end)
    rh.refit_pack(blob, prim, pos)
    assert bytes(blob) != original
    P = oa.PortOracle()
    h = P.load_pack(bytes(blob))
    lo, hi = P.primitive_bounds(h, prim)
    P.free(h)
    nodes = np.frombuffer(bytes(rh.scene_nodes(blob)), rh.NODE)
    leaf = [k for k in range(len(nodes)) if nodes["right"][k] >> 31 and nodes["left"][k] == prim]
    assert len(leaf) == 1 and np.array_equal(nodes["lo"][leaf[0]], lo) and np.array_equal(nodes["hi"][leaf[0]], hi)
    for n in nodes:
        if not n["right"] >> 31:
            l, r = nodes[int(n["left"])], nodes[int(n["right"] & 0x7fffffff)]
            assert np.array_equal(n["lo"], np.minimum(l["lo"], r["lo"])) and np.array_equal(n["hi"], np.maximum(l["hi"], r["hi"]))
    rh.set_transform(blob, prim, start, end)
    rh.refit_pack(blob, prim, pos)
    assert bytes(blob) == original

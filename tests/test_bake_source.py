"""The generated header of a baked instance (tinsel_hip_bake_source_desc, tn_host_bake.h) from scene descriptions alone -- no device: the
text is deterministic and made of integer literals only, the key follows every bit of the scene level, the scenes the plan would not give
the closed FIT instance are not bakeable and say why; and one cross-compile of cornell's baked unit for gfx950, held to the occupancy and
register figures of the kernel it replaces."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import tinsel_amd
from tinsel_amd import abi
from tinsel_amd import build as hb
from tests import oracle_api as oa


def _pack_bytes(name):
    with open(os.path.join(oa.GOLDEN, name + ".pack"), "rb") as fh:
        return fh.read()


def _plane_offset(scene, eq):
    prims = (abi.Primitive*scene.num_primitives).from_address(scene.desc.primitives)
    k = next(i for i, p in enumerate(prims) if p.type == abi.GEOM_PLANE and tuple(p.geo.plane.plane) == tuple(np.float32(v) for v in eq))
    return C.addressof(prims[k].geo.plane) - C.addressof(scene._buf)


def _edited(name, eq, new):
    raw = bytearray(_pack_bytes(name))
    off = _plane_offset(tinsel_amd.Scene(bytes(raw)), eq)
    raw[off:off + 16] = np.asarray(new, np.float32).tobytes()
    return tinsel_amd.Scene(bytes(raw))


def test_cornells_text_is_deterministic_and_keyed_by_its_sha256():
    a = tinsel_amd.Scene(_pack_bytes("cornell")).bake_source()
    b = tinsel_amd.Scene(_pack_bytes("cornell")).bake_source()
    assert a == b and a[2] and a[3] == ""
    text, key = a[0], a[1]
    assert key == hashlib.sha256(text.encode()).hexdigest()


def test_floats_are_bit_patterns():
    text = tinsel_amd.Scene(_pack_bytes("cornell")).bake_source()[0]
    body = "\n".join(l for l in text.splitlines() if not l.startswith("//") and not l.startswith("#"))
    # every number is a hexadecimal word or a plain decimal integer: with the words taken out, no '.', exponent or float suffix is left
    words = re.findall(r"\b0x[0-9a-f]+(?:ull|u)\b", body)
    rest = re.sub(r"\b0x[0-9a-f]+(?:ull|u)\b", "W", body)
    assert len(words) > 200 and all(len(w) in (11, 21) for w in words)
    assert not re.search(r"\d\.|\.\d|\d[eE][-+]?\d|\d[fF]\b", rest), "a decimal or floating literal in the generated text"
    tables = dict(re.findall(r"constexpr uint32_t (\w+)\[(\d+)\]", body))
    assert set(tables) == {"kPlaneEq", "kPlaneIdx", "kBoxes", "kPrims", "kLights", "kLightMat"}
    # cornell's ceiling, `0 -1 0 2`, by its bits
    assert "0x00000000u, 0xbf800000u, 0x00000000u, 0x40000000u" in body


def test_one_ulp_of_a_plane_coefficient_changes_the_key():
    base = tinsel_amd.Scene(_pack_bytes("cornell")).bake_source()
    up = _edited("cornell", (0.0, -1.0, 0.0, 2.0), (0.0, -1.0, 0.0, np.nextafter(np.float32(2.0), np.float32(3.0)))).bake_source()
    assert up[2] and up[1] != base[1] and up[0] != base[0]


def test_the_two_zeros_give_different_keys():
    base = tinsel_amd.Scene(_pack_bytes("cornell")).bake_source()
    neg = _edited("cornell", (0.0, -1.0, 0.0, 2.0), (-0.0, -1.0, 0.0, 2.0)).bake_source()
    assert neg[2] and neg[1] != base[1]
    # (the coefficient stands in the plane table and in the primitive's record)
    assert neg[0].count("0x80000000u") == base[0].count("0x80000000u") + 2


def _open_corner_description():
    """A floor, a left wall and a back wall -- three always-hit planes, no two of them opposing -- with a sphere light and a plain sphere in
    the corner: slim, spheres only, a flat scan whole in LDS, but open, so the plan gives its waves shading pools (plan_bounce), which the
    closed FIT set does not have.  With a ceiling over it the same scene is taken (tests/golden/make_closed.py states the rule).  Returns
    (description, what keeps its arrays alive)."""
    leaf, big = 1 << 31, 1e8
    prims = (abi.Primitive*5)()
    for p, kind in zip(prims, (abi.GEOM_PLANE, abi.GEOM_PLANE, abi.GEOM_PLANE, abi.GEOM_SPHERE, abi.GEOM_SPHERE)):
        p.type = kind
        p.start_transform.r.w = p.end_transform.r.w = 1.0
        p.start_transform.s = p.end_transform.s = 1.0
        p.material.color.x = p.material.color.y = p.material.color.z = 0.5
        p.material.roughness, p.material.eta = 0.5, 1.0
    prims[0].geo.plane.plane[:] = [0.0, 1.0, 0.0, 0.0]
    prims[1].geo.plane.plane[:] = [1.0, 0.0, 0.0, 1.0]
    prims[2].geo.plane.plane[:] = [0.0, 0.0, 1.0, 1.0]
    boxes = [((-big,)*3, (big,)*3)]*3
    for k, (x, y, radius) in ((3, (-0.25, 1.5, 0.25)), (4, (0.5, 0.5, 0.5))):
        prims[k].geo.sphere.radius = radius
        prims[k].start_transform.p.x = prims[k].end_transform.p.x = x
        prims[k].start_transform.p.y = prims[k].end_transform.p.y = y
        boxes.append(((x - radius, y - radius, -radius), (x + radius, y + radius, radius)))
    prims[3].light_samples = 1
    prims[3].material.emission.x = prims[3].material.emission.y = prims[3].material.emission.z = 10.0
    # the scene BVH: five leaves under a chain of four internal nodes (internal k: leaf k to the left, the rest to the right)
    nodes = (abi.BVHNode*9)()
    for k in range(5):
        n = nodes[4 + k]
        n.left_index, n.right_index_leaf = k, leaf
        (n.lower.x, n.lower.y, n.lower.z), (n.upper.x, n.upper.y, n.upper.z) = boxes[k]
    for k in range(4):
        nodes[k].left_index, nodes[k].right_index_leaf = 4 + k, (k + 1 if k < 3 else 8)
        (nodes[k].lower.x, nodes[k].lower.y, nodes[k].lower.z), (nodes[k].upper.x, nodes[k].upper.y, nodes[k].upper.z) = boxes[0]
    desc = abi.SceneDesc()
    desc.primitives, desc.num_primitives = C.cast(prims, C.c_void_p), 5
    desc.bvh_nodes, desc.num_bvh_nodes = C.cast(nodes, C.c_void_p), 9
    return desc, (prims, nodes)


def _description_bake_source(desc):
    from tinsel_amd import renderer
    L = tinsel_amd.load_library()
    return renderer._bake_source(lambda buf, cap, k, good: L.tinsel_hip_bake_source_desc(C.byref(desc), None, buf, cap, k, good))


@pytest.mark.parametrize("name, reason", [
    ("glass", "does not run the fused pipeline"),
    ("veach", "defers its mesh walks"),
    ("features", "not slim"),
    ("cornell_probe", "not slim"),
    ("open-corner", "the scene's features lie outside the closed FIT set"),
])
def test_scenes_the_plan_gives_another_kernel_are_not_bakeable(name, reason):
    if name == "open-corner":           # (three planes without an opposing pair: made here, no pack holds it)
        desc, keep = _open_corner_description()
        L = tinsel_amd.load_library()
        assert L.tinsel_hip_scene_features(C.byref(desc)) == abi.BOUNCE_SPHERE and L.tinsel_hip_scene_slim(C.byref(desc))
        text, key, ok, why = _description_bake_source(desc)
    else:
        text, key, ok, why = tinsel_amd.Scene(_pack_bytes(name)).bake_source()
    assert not ok and why.startswith("bake_source: not bakeable: ") and key == hashlib.sha256(text.encode()).hexdigest()
    assert reason in why


def _env_loft_description():
    """tests/golden/scenes/env_loft.tin.in as a scene description made here (its pack embeds a 31-MB probe and is generated, not committed;
    tests/test_bounce_fit.py::test_the_scene_bits_of_env_loft makes the same scene for the feature bits alone): a plane, a quad light, three
    spheres and a four-triangle tetrahedron under a probe -- here with everything create's host half reads: vertices, normals, indices,
    trees with boxes, cdfs, a 2 x 2 probe with its tables and a hand-made scene BVH.  Returns (description, what keeps its arrays alive)."""
    leaf = 1 << 31
    keep = []

    def arr(kind, values):
        a = (kind*len(values))(*values)
        keep.append(a)
        return a

    def tree(shape, lo, hi):
        nodes = (abi.BVHNode*len(shape))()
        for n, (left, right) in zip(nodes, shape):
            n.left_index, n.right_index_leaf = left, right
            (n.lower.x, n.lower.y, n.lower.z), (n.upper.x, n.upper.y, n.upper.z) = lo, hi
        keep.append(nodes)
        return nodes

    def mesh(p, ident, verts, tris, shape):
        lo, hi = tuple(min(v[c] for v in verts) for c in range(3)), tuple(max(v[c] for v in verts) for c in range(3))
        g = p.geo.mesh
        g.positions = C.cast(arr(C.c_float, [c for v in verts for c in v]), C.c_void_p)
        g.normals = C.cast(arr(C.c_float, [0.0, 1.0, 0.0]*len(verts)), C.c_void_p)
        g.indices = C.cast(arr(C.c_int32, [i for t in tris for i in t]), C.c_void_p)
        nodes = tree(shape, lo, hi)
        g.nodes, g.num_nodes = C.cast(nodes, C.c_void_p), len(nodes)
        g.cdf = C.cast(arr(C.c_float, [(k + 1)/len(tris) for k in range(len(tris))]), C.c_void_p)
        g.num_vertices, g.num_indices, g.area, g.id = len(verts), 3*len(tris), 1.0, ident
        return lo, hi

    kinds = (abi.GEOM_PLANE, abi.GEOM_MESH, abi.GEOM_SPHERE, abi.GEOM_SPHERE, abi.GEOM_SPHERE, abi.GEOM_MESH)
    prims = (abi.Primitive*6)()
    keep.append(prims)
    for p, kind in zip(prims, kinds):
        p.type = kind
        p.start_transform.r.w = p.end_transform.r.w = 1.0
        p.start_transform.s = p.end_transform.s = 1.0
        p.material.color.x = p.material.color.y = p.material.color.z = 0.5
        p.material.roughness, p.material.eta = 0.5, 1.0
    big = 1e8
    boxes = [((-big,)*3, (big,)*3)]
    prims[0].geo.plane.plane[:] = [0.0, 1.0, 0.0, 0.0]
    boxes.append(mesh(prims[1], 1, [(-1.0, 3.0, -1.0), (1.0, 3.0, -1.0), (1.0, 3.0, 1.0), (-1.0, 3.0, 1.0)], [(0, 1, 2), (0, 2, 3)],
                      [(1, 2), (0, leaf), (1, leaf)]))                              # the quad light: one internal node over two triangles
    prims[1].light_samples = 1
    prims[1].material.emission.x = prims[1].material.emission.y = prims[1].material.emission.z = 10.0
    for k, x in ((2, -2.0), (3, 0.0), (4, 2.0)):
        prims[k].geo.sphere.radius = 0.5
        prims[k].start_transform.p.x = prims[k].end_transform.p.x = x
        prims[k].start_transform.p.y = prims[k].end_transform.p.y = 0.5
        boxes.append(((x - 0.5, 0.0, -0.5), (x + 0.5, 1.0, 0.5)))
    boxes.append(mesh(prims[5], 2, [(3.0, 0.0, 0.0), (4.0, 0.0, 0.0), (3.5, 0.0, 1.0), (3.5, 1.0, 0.5)],
                      [(0, 1, 2), (0, 1, 3), (1, 2, 3), (2, 0, 3)],
                      [(1, 2), (3, 4), (5, 6), (0, leaf), (1, leaf), (2, leaf), (3, leaf)]))      # four triangles: a real walk
    # the scene BVH: six leaves under a chain of five internal nodes (internal k: leaf k to the left, the rest to the right)
    scene = (abi.BVHNode*11)()
    keep.append(scene)
    for k in range(6):
        n = scene[5 + k]
        n.left_index, n.right_index_leaf = k, leaf
        (n.lower.x, n.lower.y, n.lower.z), (n.upper.x, n.upper.y, n.upper.z) = boxes[k]
    for k in range(5):
        scene[k].left_index, scene[k].right_index_leaf = 5 + k, (k + 1 if k < 4 else 10)
        (scene[k].lower.x, scene[k].lower.y, scene[k].lower.z), (scene[k].upper.x, scene[k].upper.y, scene[k].upper.z) = boxes[0]
    desc = abi.SceneDesc()
    desc.primitives, desc.num_primitives = C.cast(prims, C.c_void_p), 6
    desc.bvh_nodes, desc.num_bvh_nodes = C.cast(scene, C.c_void_p), 11
    desc.probe_valid, desc.probe_width, desc.probe_height = 1, 2, 2
    desc.probe_data = C.cast(arr(C.c_float, [1.0]*16), C.c_void_p)
    desc.probe_pdf_x = C.cast(arr(C.c_float, [0.5]*4), C.c_void_p)
    desc.probe_cdf_x = C.cast(arr(C.c_float, [0.5, 1.0]*2), C.c_void_p)
    desc.probe_pdf_y = C.cast(arr(C.c_float, [0.5]*2), C.c_void_p)
    desc.probe_cdf_y = C.cast(arr(C.c_float, [0.5, 1.0]), C.c_void_p)
    return desc, keep


def test_env_loft_is_not_bakeable():
    from tinsel_amd import renderer
    L = tinsel_amd.load_library()
    desc, keep = _env_loft_description()
    assert L.tinsel_hip_scene_features(C.byref(desc)) == abi.BOUNCE_PROBE | abi.BOUNCE_SPHERE | abi.BOUNCE_MESH_WALK
    text, key, ok, why = renderer._bake_source(lambda buf, cap, k, good: L.tinsel_hip_bake_source_desc(C.byref(desc), None, buf, cap, k, good))
    assert not ok and why.startswith("bake_source: not bakeable: ") and "not slim" in why, why
    assert key == hashlib.sha256(text.encode()).hexdigest() and "constexpr int kNumPrims = 6;" in text


def test_bounce_bake_travels_beside_the_tuning_struct():
    """the bake mode is a setting of its own (tinsel_hip_set_bounce_bake): tinsel_hip_tuning keeps its layout, abi.Tuning carries the mode"""
    t = abi.Tuning()
    assert C.sizeof(abi.Tuning) == 128 and "bounce_bake" not in [f for f, _ in abi.Tuning._fields_] and abi.Tuning.BINDING_FIELDS == ("bounce_bake",)
    assert t.bounce_bake == -1 and abi.Tuning(bounce_bake=0).bounce_bake == 0 and t.replace(bounce_bake=1).bounce_bake == 1
    assert abi.Tuning(bounce_bake=0).replace(plane_pairs=0).bounce_bake == 0 and abi.Tuning(bounce_bake=1).as_dict()["bounce_bake"] == 1
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tinsel_hip.h")).read()
    body = hdr[hdr.index("typedef struct tinsel_hip_tuning {"):hdr.index("} tinsel_hip_tuning;")]
    assert "bounce_bake" not in body and "int tinsel_hip_set_bounce_bake(tinsel_hip* r, int mode);" in hdr


def test_bounce_fit_off_is_not_bakeable():
    _, _, ok, why = tinsel_amd.Scene(_pack_bytes("cornell")).bake_source(abi.Tuning(bounce_fit=0))
    assert not ok and "bounce_fit" in why


def test_bake_refuses_a_kernel_that_is_not_at_the_closed_instances_occupancy():
    ok = {"waves_per_simd": 4, "scratch_bytes": 0, "vgprs": 104, "sgpr_spills": 17}
    assert hb.baked_refusal(ok) is None and hb.baked_refusal(dict(ok, vgprs=128)) is None
    for bad in (dict(ok, waves_per_simd=3, vgprs=136), dict(ok, waves_per_simd=5, vgprs=91), dict(ok, scratch_bytes=16), None, {}):
        assert hb.baked_refusal(bad)


def test_bake_refuses_a_key_that_is_not_the_texts():
    image, why = hb.bake("// nothing\n", "0"*64)
    assert image is None and "sha256" in why


def test_cornells_baked_unit_cross_compiles_within_the_closed_instances_budget():
    """From -Rpass-analysis=kernel-resource-usage: four waves per SIMD, no scratch, VGPRs <= 128, and strictly fewer spilled scalars than
    the library's k_bounce<2,1,0> of the same build (csrc/_obj/resources.json)."""
    text, key, ok, _ = tinsel_amd.Scene(_pack_bytes("cornell")).bake_source()
    assert ok
    with open(os.path.join(hb.OBJ_DIR, "resources.json")) as f:
        lib = json.load(f)["kernels"]["k_bounce<2,1,0>"]
    with tempfile.TemporaryDirectory(prefix="tinsel_bake_test_") as tmp:
        header = os.path.join(tmp, "scene.h")
        with open(header, "w") as f:
            f.write(text)
        cmd = hb.bake_command(hb.hipcc(), header, "baked.co", extra=["-Rpass-analysis=kernel-resource-usage"])
        p = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-3000:]
        res = hb._parse_resources(p.stderr)["k_bounce<2,1,0>"]
        res["code_bytes"] = hb._code_bytes(os.path.join(tmp, "baked.co")).get("k_bounce<2,1,0>")
    print("baked k_bounce<2,1,0>:", json.dumps(res, sort_keys=True), "| library:", json.dumps(lib, sort_keys=True))
    assert res["waves_per_simd"] == 4 and res["scratch_bytes"] == 0 and res["vgprs"] <= 128
    assert res["sgpr_spills"] < lib["sgpr_spills"]

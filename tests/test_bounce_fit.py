"""k_bounce's FIT instances (tn_fused.h: the fused kernel compiled for a fixed set of scene and plan features), as the compiler reported
them for THIS build (tinsel_amd/csrc/_obj/resources.json, written by __graft_entry__.build(); `code_bytes` is the size of the kernel's
function symbol in the gfx950 code object).  A FIT instance exists to be SMALLER than the general kernel it stands in for -- in code, in
registers, in scratch -- and must keep the four waves per SIMD every measured number of the fused pipeline rests on.  No GPU needed."""
import hashlib
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "tinsel_amd", "csrc", "_obj")

# instance -> the general kernel it replaces (same LDS / DEFER arguments)
FIT = {"k_bounce<2,1,0>": "k_bounce<0,1,0>", "k_bounce<3,1,1>": "k_bounce<0,1,1>"}


def _resources():
    path = os.path.join(OBJ, "resources.json")
    obj = os.path.join(OBJ, "tinsel_hip.o")
    if not (os.path.exists(path) and os.path.exists(obj)):
        pytest.skip("no build record in this tree (python -c 'import __graft_entry__ as g; g.build()' writes it)")
    rec = json.load(open(path))
    if rec.get("object_sha256") != hashlib.sha256(open(obj, "rb").read()).hexdigest() or not rec.get("kernels"):
        pytest.skip("resources.json does not describe the object the library was linked from")
    return rec["kernels"]


def test_every_kernel_has_its_code_size():
    k = _resources()
    assert all(v.get("code_bytes", 0) > 0 for v in k.values()), [n for n, v in k.items() if not v.get("code_bytes")][:3]


def test_the_fit_instances_are_the_ones_the_launch_table_names():
    k = _resources()
    assert sorted(n for n in k if n.startswith("k_bounce<") and int(n[len("k_bounce<"):].split(",")[0]) >= 2) == sorted(FIT)


@pytest.mark.parametrize("fit", sorted(FIT))
def test_a_fit_instance_keeps_four_waves_and_is_smaller_than_its_general_kernel(fit):
    k = _resources()
    f, g = k[fit], k[FIT[fit]]
    assert f["waves_per_simd"] == 4 and f["vgprs"] <= 128, f
    assert f["scratch_bytes"] <= g["scratch_bytes"], (f, g)
    assert f["code_bytes"] < g["code_bytes"], (f["code_bytes"], g["code_bytes"])


def test_the_closed_scene_instance_fits_the_instruction_cache():
    """64 KB of instruction cache shared by two CUs (AMD's CDNA3 white paper; assumed unchanged for CDNA4)"""
    assert _resources()["k_bounce<2,1,0>"]["code_bytes"] < 65536


def test_the_build_reads_code_sizes_from_a_bundled_code_object(tmp_path):
    """build.py's _code_bytes on a hand-made clang offload bundle around a minimal ELF64 with one function symbol"""
    import struct
    import sys
    sys.path.insert(0, ROOT)
    from tinsel_amd import build as hb
    name = b"_ZN2tn8k_bounceILi2ELb1ELb0EEEvNS_14BounceKernargsE"
    strtab = b"\0" + name + b"\0"
    sym = struct.pack("<IBBHQQ", 0, 0, 0, 0, 0, 0) + struct.pack("<IBBHQQ", 1, 0x12, 0, 1, 0x1000, 49008)
    ehdr_size, sh_size = 64, 64
    off_sym, off_str = ehdr_size, ehdr_size + len(sym)
    shoff = off_str + len(strtab)
    sh = lambda name, kind, off, size, link, entsize: struct.pack("<IIQQQQIIQQ", name, kind, 0, 0, off, size, link, 0, 1, entsize)
    sections = sh(0, 0, 0, 0, 0, 0) + sh(0, 1, 0, 0, 0, 0) + sh(0, 2, off_sym, len(sym), 3, 24) + sh(0, 3, off_str, len(strtab), 0, 0)
    ehdr = b"\x7fELF\x02\x01\x01" + b"\0"*9 + struct.pack("<HHIQQQIHHHHHH", 1, 224, 1, 0, 0, shoff, 0, ehdr_size, 0, 0, sh_size, 4, 0)
    elf = ehdr + sym + strtab + sections
    triple = b"hipv4-amdgcn-amd-amdhsa--gfx950"
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    head = magic + struct.pack("<Q", 1)
    entry_len = 24 + len(triple)
    bundle = head + struct.pack("<QQQ", len(head) + entry_len, len(elf), len(triple)) + triple + elf
    for blob in (elf, bundle):
        path = tmp_path / "dev.o"
        path.write_bytes(blob)
        assert hb._code_bytes(str(path)) == {"k_bounce<2,1,0>": 49008}


# ---- the scene's feature bits, from the scene description alone (tinsel_hip_scene_features: no device, no renderer) ----------------------

def _bits():
    from tinsel_amd import abi
    return abi


PACK_BITS = {           # tests/golden/<name>.pack -> what its primitives, materials and meshes ask of the fused kernel
    "cornell": ("SPHERE",),                                                         # five planes, a quad light, two spheres
    "veach": ("SPHERE",),                                                           # two planes, three quads, four sphere lights
    "gloss": ("SPHERE",),
    "glass": ("SPHERE", "TRANSMISSION", "MESH_WALK"),                               # a 12- and a 1280-triangle mesh of glass
    "motionblur": ("SPHERE", "MOTION", "MESH_WALK"),                                # a moving 10 214-triangle mesh
    "features": ("SPHERE", "MOTION", "MEDIA", "TRANSMISSION", "MESH_WALK"),
    "cornell_probe": ("SPHERE", "PROBE"),
    "anim_cornell_0": ("SPHERE", "MOTION"),
}


@pytest.mark.parametrize("name", sorted(PACK_BITS))
def test_the_scene_bits_of_a_pack(name):
    import tinsel_amd
    abi = _bits()
    scene = tinsel_amd.Scene.load_pack(os.path.join(ROOT, "tests", "golden", name + ".pack"))
    want = 0
    for b in PACK_BITS[name]:
        want |= getattr(abi, "BOUNCE_" + b)
    assert scene.bounce_features() == want


def test_the_scene_bits_of_env_loft():
    """tests/golden/scenes/env_loft.tin.in as a scene description (its pack embeds a 31-MB probe and is generated, not committed): a
    plane, a quad light, three spheres and a four-triangle tetrahedron under a probe.  Only what the derivation reads is filled in: the
    probe flag, the primitive kinds, their transforms and materials, and each mesh tree's shape."""
    import ctypes as C
    import tinsel_amd
    abi = _bits()
    L = tinsel_amd.load_library()
    leaf = 1 << 31

    def tree(shape):
        nodes = (abi.BVHNode*len(shape))()
        for n, (left, right) in zip(nodes, shape):
            n.left_index, n.right_index_leaf = left, right
        return nodes
    quad = tree([(1, 2), (0, leaf), (1, leaf)])                                             # one internal node over two triangles
    tetra = tree([(1, 2), (3, 4), (5, 6), (0, leaf), (1, leaf), (2, leaf), (3, leaf)])      # four triangles: a real walk
    prims = (abi.Primitive*6)()
    for p, kind in zip(prims, (abi.GEOM_PLANE, abi.GEOM_MESH, abi.GEOM_SPHERE, abi.GEOM_SPHERE, abi.GEOM_SPHERE, abi.GEOM_MESH)):
        p.type = kind
        p.start_transform.r.w = p.end_transform.r.w = 1.0
        p.start_transform.s = p.end_transform.s = 1.0
    for p, nodes in ((prims[1], quad), (prims[5], tetra)):
        p.geo.mesh.nodes = C.cast(nodes, C.c_void_p)
        p.geo.mesh.num_nodes = len(nodes)
    prims[1].light_samples = 1
    desc = abi.SceneDesc()
    desc.primitives, desc.num_primitives, desc.probe_valid = C.cast(prims, C.c_void_p), 6, 1
    assert L.tinsel_hip_scene_features(C.byref(desc)) == abi.BOUNCE_PROBE | abi.BOUNCE_SPHERE | abi.BOUNCE_MESH_WALK
    prims[5].geo.mesh.nodes, prims[5].geo.mesh.num_nodes = C.cast(quad, C.c_void_p), 3      # (a quad in its place: nothing left to walk)
    prims[3].end_transform.p.x = 0.25                                                       # (and a sphere that moves)
    assert L.tinsel_hip_scene_features(C.byref(desc)) == abi.BOUNCE_PROBE | abi.BOUNCE_SPHERE | abi.BOUNCE_MOTION

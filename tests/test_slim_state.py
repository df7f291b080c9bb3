"""The SLIM path state of k_bounce's FIT instances (tn_path_state.h load_state_slim, tn_fused.h): which scenes carry it -- the host's
predicate from a scene description alone (tinsel_hip_scene_slim: no device, no renderer) -- and what the instances cost as the compiler
reported them for THIS build (tinsel_amd/csrc/_obj/resources.json) against the record of the build before them
(profiles/r09_resources.md).  No GPU needed."""
import ctypes as C
import hashlib
import json
import os
import struct

import pytest

import tinsel_amd
from tinsel_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OBJ = os.path.join(ROOT, "tinsel_amd", "csrc", "_obj")


def _scene(name):
    return tinsel_amd.Scene.load_pack(os.path.join(GOLDEN, name + ".pack"))


def _prims(scene):
    return (abi.Primitive*scene.num_primitives).from_address(scene.desc.primitives)


# ---- the predicate ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,slim", [("cornell", True), ("veach", True), ("gloss", True),
                                       ("features", False), ("glass", False), ("anim_cornell_0", False), ("cornell_probe", False)])
def test_which_packs_are_slim(name, slim):
    assert _scene(name).bounce_slim() is slim


def test_no_reference_pack_of_the_slim_set_has_subsurface():
    for name in ("cornell", "veach", "gloss"):
        assert all(struct.pack("<f", p.material.subsurface) == b"\0\0\0\0" for p in _prims(_scene(name))), name


@pytest.mark.parametrize("value", [0.25, -0.0, 1e-45, float("nan")], ids=["0.25", "minus-zero", "denormal", "nan"])
def test_one_material_with_subsurface_takes_the_scene_out(value):
    """+0.0f by its BITS: -0.0f compares equal to it and is still not slim; the feature bits do not know about subsurface"""
    scene = _scene("cornell")
    bits = scene.bounce_features()
    prims = _prims(scene)
    for k in (0, len(prims) - 1):
        assert scene.bounce_slim()
        prims[k].material.subsurface = value
        assert not scene.bounce_slim() and scene.bounce_features() == bits
        prims[k].material.subsurface = 0.0
    assert scene.bounce_slim()


def test_nothing_to_look_at_is_not_slim():
    L = tinsel_amd.load_library()
    assert L.tinsel_hip_scene_slim(None) == 0
    assert L.tinsel_hip_scene_slim(C.byref(abi.SceneDesc())) == 0


# ---- the instances' resources -----------------------------------------------------------------------------------------------------------

# profiles/r09_resources.md: the FIT instances of the build before the slim state
PARENT = {
    "k_bounce<2,1,0>": dict(vgprs=116, sgpr_spills=65, scratch_bytes=0, code_bytes=49008),
    "k_bounce<3,1,1>": dict(vgprs=128, sgpr_spills=98, scratch_bytes=20, code_bytes=61992),
}


def _resources():
    path = os.path.join(OBJ, "resources.json")
    obj = os.path.join(OBJ, "tinsel_hip.o")
    if not (os.path.exists(path) and os.path.exists(obj)):
        pytest.skip("no build record in this tree (python -c 'import __graft_entry__ as g; g.build()' writes it)")
    rec = json.load(open(path))
    if rec.get("object_sha256") != hashlib.sha256(open(obj, "rb").read()).hexdigest() or not rec.get("kernels"):
        pytest.skip("resources.json does not describe the object the library was linked from")
    return rec["kernels"]


@pytest.mark.parametrize("fit", sorted(PARENT))
def test_a_slim_instance_costs_no_more_than_the_one_before_it(fit):
    k, was = _resources()[fit], PARENT[fit]
    print(fit, {f: k[f] for f in ("waves_per_simd", "vgprs", "sgpr_spills", "scratch_bytes", "code_bytes")}, "was", was)
    assert k["waves_per_simd"] == 4
    assert k["scratch_bytes"] <= was["scratch_bytes"]
    assert k["vgprs"] <= was["vgprs"] and k["sgpr_spills"] <= was["sgpr_spills"]
    assert k["code_bytes"] < was["code_bytes"]

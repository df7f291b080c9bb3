"""Opposing plane pairs of the flat scan's plane table, without a device: the host's pairing rule through tinsel_hip_scene_plane_pairs
(committed packs and edited scene descriptions), and tn_plane.h -- the text the kernels compile -- built for the host on its own and held
to two IntersectRayPlane calls bit for bit (tests/plane_pairs_host.cpp, run as a child process)."""
import os
import subprocess

import numpy as np
import pytest

import tinsel_amd
from tinsel_amd import abi
from tests.oracle_api import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scene(name):
    return tinsel_amd.Scene.load_pack(os.path.join(GOLDEN, name + ".pack"))


def _planes(scene):
    prims = (abi.Primitive*scene.num_primitives).from_address(scene.desc.primitives)
    return prims, [i for i, p in enumerate(prims) if p.type == abi.GEOM_PLANE]


def _eq(prims, i):
    return tuple(prims[i].geo.plane.plane)


def _set(prims, i, eq):
    for k, v in enumerate(eq):
        prims[i].geo.plane.plane[k] = v


def _find(prims, planes, eq):
    return next(i for i in planes if _eq(prims, i) == tuple(np.float32(v) for v in eq))


def test_cornell_has_two_pairs_and_a_single():
    scene = _scene("cornell")
    prims, planes = _planes(scene)
    assert len(planes) == 5
    pairs, singles = scene.plane_pairs()
    x = (_find(prims, planes, (1, 0, 0, 1)), _find(prims, planes, (-1, 0, 0, 1)))
    y = (_find(prims, planes, (0, 1, 0, 0)), _find(prims, planes, (0, -1, 0, 2)))
    assert sorted(pairs) == sorted([tuple(sorted(x)), tuple(sorted(y))]) and singles == 1
    assert all(a < b for a, b in pairs) and pairs == sorted(pairs)


def test_glass_has_its_floor_and_ceiling():
    scene = _scene("glass")
    prims, planes = _planes(scene)
    pairs, singles = scene.plane_pairs()
    assert pairs and singles == len(planes) - 2*len(pairs)
    floor_ceiling = [(a, b) for a, b in pairs if _eq(prims, a)[1] != 0.0]
    assert len(floor_ceiling) == 1
    for a, b in pairs:
        na, nb = _eq(prims, a)[:3], _eq(prims, b)[:3]
        assert all(x == -y for x, y in zip(na, nb)), (na, nb)


def test_a_scene_without_opposing_planes_has_no_pair():
    """(the RULE on the description: whether a renderer of the scene has a table at all is create's business, tests/test_gpu_plane_pairs.py)"""
    for name in ("veach", "many_spheres"):
        scene = _scene(name)
        prims, planes = _planes(scene)
        eqs = [_eq(prims, i) for i in planes]
        expect = any(all(x == -y for x, y in zip(a[:3], b[:3])) for k, a in enumerate(eqs) for b in eqs[k + 1:])
        pairs, singles = scene.plane_pairs()
        assert bool(pairs) == expect and 2*len(pairs) + singles <= len(planes), name


def _edited(a_eq, b_eq, third=None):
    """cornell with its floor / ceiling rewritten (and optionally the single plane): (pairs, singles, floor, ceiling, single)"""
    scene = _scene("cornell")
    prims, planes = _planes(scene)
    fl, ce = _find(prims, planes, (0, 1, 0, 0)), _find(prims, planes, (0, -1, 0, 2))
    x = {_find(prims, planes, (1, 0, 0, 1)), _find(prims, planes, (-1, 0, 0, 1))}
    single, = [i for i in planes if i not in x and i not in (fl, ce)]
    _set(prims, fl, a_eq)
    _set(prims, ce, b_eq)
    if third is not None:
        _set(prims, single, third)
    pairs, singles = scene.plane_pairs()
    return pairs, singles, fl, ce, single


def test_scaled_normals_and_signed_zeros_pair():
    for a, b in (((0.0, 2.0, 0.0, 0.0), (0.0, -2.0, 0.0, 4.0)), ((0.0, 1.0, 0.0, 0.0), (-0.0, -1.0, -0.0, 2.0)), ((-0.0, 1.0, 0.0, 0.5), (-0.0, -1.0, 0.0, -0.5))):
        pairs, singles, fl, ce, _ = _edited(a, b)
        assert tuple(sorted((fl, ce))) in pairs and len(pairs) == 2 and singles == 1, (a, b)


def test_one_ulp_off_a_nan_or_an_infinity_do_not_pair():
    up = float(np.nextafter(np.float32(1.0), np.float32(2.0)))
    cases = [((0.0, 1.0, 0.0, 0.0), (0.0, -up, 0.0, 2.0)),
             ((0.0, 1.0, 0.0, 0.0), (1e-45, -1.0, 0.0, 2.0)),                   # a denormal is not a zero
             ((0.0, 1.0, 0.0, float("nan")), (0.0, -1.0, 0.0, 2.0)),
             ((0.0, 1.0, 0.0, 0.0), (0.0, -1.0, 0.0, float("inf"))),
             ((0.0, float("inf"), 0.0, 0.0), (0.0, float("-inf"), 0.0, 2.0)),
             ((0.0, 1.0, 0.0, 0.0), (0.0, 1.0, 0.0, 2.0))]                      # parallel, facing the same way
    for a, b in cases:
        pairs, singles, fl, ce, _ = _edited(a, b)
        assert len(pairs) == 1 and singles == 3 and fl not in pairs[0] and ce not in pairs[0], (a, b)


def test_three_parallel_planes_make_one_pair_and_one_single():
    pairs, singles, fl, ce, single = _edited((0.0, 1.0, 0.0, 0.0), (0.0, -1.0, 0.0, 2.0), third=(0.0, 1.0, 0.0, 1.0))
    ys = sorted((fl, ce, single))
    # greedily in primitive order: the first of the three pairs with the first one after it that opposes it (the ceiling opposes both
    # others, which do not oppose each other); no plane twice
    want = (ys[0], ce) if ys[0] != ce else (ce, ys[1])
    assert len(pairs) == 2 and singles == 1 and want in pairs, (pairs, ys)
    assert len({i for p in pairs for i in p}) == 4


def test_the_tuning_struct_ends_with_plane_pairs():
    t = abi.Tuning()
    assert abi.Tuning._fields_[-1][0] == "plane_pairs" and t.plane_pairs == -1 and abi.Tuning(plane_pairs=0).plane_pairs == 0
    hdr = open(os.path.join(ROOT, "include", "tinsel_hip.h")).read()
    body = hdr[hdr.index("typedef struct tinsel_hip_tuning {"):hdr.index("} tinsel_hip_tuning;")]
    assert body.rstrip().splitlines()[-1].split()[1].rstrip(";") == "plane_pairs"


def test_the_paired_test_equals_two_plane_tests_bit_for_bit(tmp_path):
    """2^28 random (origin, direction, pair) triples and the directed cases of tests/plane_pairs_host.cpp: hit flags, t, chosen plane and
    normal bits.  Built with -ffp-contract=off like the library; the program is a plain host binary (it may be built with
    -fsanitize=address,undefined as it is).  About 40 core-seconds: 9 s of wall time on eight cores, the longest test of the no-device
    suite -- 2^28 is the count this check was given, and the program spreads it over the host's cores (16 at the most)."""
    exe = tmp_path / "plane_pairs_host"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-I", os.path.join(ROOT, "tinsel_amd", "csrc"),
                    "-o", str(exe), os.path.join(ROOT, "tests", "plane_pairs_host.cpp")], check=True)
    p = subprocess.run([str(exe), "28", str(max(1, min(16, os.cpu_count() or 1)))], capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    words = p.stdout.split()
    assert int(words[words.index("random") + 1]) >= 1 << 28 and int(words[words.index("directed") + 1]) > 1_000_000
    assert words[-2:] == ["mismatches", "0"]
    # every branch was taken, in numbers: both ahead (the kernel's fallback), A chosen, B chosen, no hit
    import re
    counts = [int(v) for v in re.findall(r"\d+", p.stdout[p.stdout.index("random"):])]
    assert len(counts) == 6 and all(c > 1 << 20 for c in counts[1:5]), p.stdout

#!/usr/bin/env python3
"""Exact-tie corpus: tests/golden/ties.golden.npz.

Six small scenes in which two surfaces coincide -- primitives defined twice, mesh instances placed twice, quads lying in a plane or in
each other, one triangle repeated inside a mesh -- so that almost every ray has two hits with the same t and only the visit order of
the reference's Trace() (render.cpp:17-62: QueryBVH over the scene tree, strict `t < minT`, the first visit wins) names the winner.
Each scene is written as .tin text, loaded by the reference's own loader + Scene::Build, and the file keeps per scene: the pack (as
bytes), the camera rays, Trace()'s records (primitive, t, normal) for the scene's rays, the set of primitives that attain each ray's
minimum (from PrimitiveIntersect per primitive), and the per-path radiance and framebuffer of 2 seeded passes -- so the GPU box needs
neither the reference nor the .tin.  Needs the reference (oracle/_ref).

The rays themselves are not stored (random floats do not compress, and the file is held to the size of fuzz.golden.npz): all_rays(name, g)
below makes them again from a seed, with Generator.random / integers and float32 arithmetic only, and the file keeps their CRC-32.

Usage:  python tests/golden/make_ties.py            (deterministic: the same file every time; prints the table of tests/test_ties.py)"""
import io
import os
import sys
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F = np.float32
SCENES = ["dup_flat", "dup_order", "dup_moving", "dup_scene_bvh", "dup_walked", "dup_triangles"]
W, H = 24, 16
PASSES = 2
N_AIMED, N_AXIS, N_SURFACE = 5120, 768, 1536            # + W*H camera rays = 7,808 rays per scene
FLOOR_TIED, FLOOR_NOT_LOWEST, FLOOR_NEAR = 1000, 500, 100

MESHES = """
mesh quad
{
	verts 4
	-0.5 0 0.5
	0.5 0 0.5
	0.5 0 -0.5
	-0.5 0 -0.5

	tris 2
	0 2 1
	0 3 2
}

mesh pyramid
{
	verts 5
	-1 0 -1
	1 0 -1
	1 0 1
	-1 0 1
	0 1.5 0

	tris 6
	1 0 4
	2 1 4
	3 2 4
	0 3 4
	0 1 2
	0 2 3
}
"""

# the pyramid with two faces repeated on vertices of their own (5..7: the -z face, 8..10: the +z face).  `which`: "both" (the corpus's mesh: one
# repeat ahead of its original in the triangle list, one behind), "originals", "repeats" (the repeats in place of their originals), "neither" --
# the last three only tell the generator which triangle of a pair a ray's normal came from.
_PYR_VERTS = ["-1 0 -1", "1 0 -1", "1 0 1", "-1 0 1", "0 1.5 0", "-1 0 -1", "1 0 -1", "0 1.5 0", "1 0 1", "-1 0 1", "0 1.5 0"]
_PYR_REST = ["2 1 4", "0 3 4", "0 1 2", "0 2 3"]
_PYR_TRIS = ["1 0 4", "2 1 4", "3 2 4", "0 3 4", "0 1 2", "0 2 3"]


def pyramid_repeated(which):
    tris = {"both": ["9 8 10", "1 0 4"] + _PYR_REST[:1] + ["3 2 4"] + _PYR_REST[1:] + ["6 5 7"],
            "originals": ["1 0 4"] + _PYR_REST[:1] + ["3 2 4"] + _PYR_REST[1:],
            "repeats": ["9 8 10"] + _PYR_REST + ["6 5 7"],
            "neither": list(_PYR_REST)}.get(which)
    verts = list(_PYR_VERTS)
    if tris is None:
        # "tri0" .. "tri5": ONE of the pyramid's six triangles (and a speck far below everything, so that the tree has two leaves)
        verts += ["1000 -1000 1000", "1000.001 -1000 1000", "1000 -1000 1000.001"]
        tris = [_PYR_TRIS[int(which[3:])], "11 12 13"]
    return "mesh pyramid2\n{\n\tverts %d\n%s\n\n\ttris %d\n%s\n}\n" % (
        len(verts), "\n".join("\t" + v for v in verts), len(tris), "\n".join("\t" + t for t in tris))


MATERIALS = [("red", "0.8 0.2 0.15", 0.6, 0.0), ("green", "0.2 0.75 0.25", 0.3, 0.0), ("blue", "0.2 0.3 0.85", 0.1, 0.0),
             ("gold", "0.9 0.7 0.3", 0.25, 1.0), ("white", "0.85 0.85 0.85", 1.0, 0.0), ("grey", "0.4 0.4 0.4", 0.5, 0.0)]


def header(depth, cam_pos, cam_target, shutter):
    out = ["options", "{", "\twidth %d" % W, "\theight %d" % H, "\tmaxDepth %d" % depth, "\tfilter gaussian 1 1.5", "}", "",
           "camera", "{", "\tposition %s" % cam_pos, "\ttarget %s" % cam_target, "\tfov 45"]
    if shutter:
        out += ["\tshutterstart 0", "\tshutterend 1"]
    out += ["}", "", "sky", "{", "\thorizon 0.5 0.55 0.6", "\tzenith 0.25 0.35 0.6", "}", ""]
    for name, color, rough, metal in MATERIALS:
        out += ["material %s" % name, "{", "\tcolor %s" % color, "\troughness %g" % rough, "\tspecular 0.5", "\tmetallic %g" % metal, "}", ""]
    out += ["material light", "{", "\temission 12 11 9", "\tcolor 0 0 0", "}", ""]
    return "\n".join(out)


def prim(kind, mat, pos=None, rot=None, scale=None, radius=None, plane=None, mesh=None, light=0):
    out = ["primitive", "{", "\ttype %s" % kind]
    if plane:
        out.append("\tplane %s" % plane)
    if pos:
        out.append("\tposition %s" % pos)
    if rot:
        out.append("\trotation %s" % rot)
    if scale:
        out.append("\tscale %s" % scale)
    if radius:
        out.append("\tradius %s" % radius)
    if mesh:
        out.append("\tmesh %s" % mesh)
    out.append("\tmaterial %s" % mat)
    if light:
        out.append("\tlightSamples %d" % light)
    out.append("}")
    return "\n".join(out)


def twice(mats, kind, **kw):
    return [prim(kind, mats[0], **kw), prim(kind, mats[1], **kw)]


LIGHT = dict(pos="0 3.5 0", rot="1 0 0 0", scale="1.5", mesh="quad", light=1)        # a quad turned to face down (x, y, z, w)
ROT_Y = "0 0.382683 0 0.92388"                                                            # 45 degrees about y
ROT_A = "0.258819 0 0 0.965926"                                                           # 30 degrees about x


def scene_text(name, pyramid2="both"):
    """-> (.tin text, aim boxes [(lo, hi)]: where the scene's rays are aimed, origin box (lo, hi))"""
    aims = []
    box = lambda c, h: (np.array(c, np.float64) - np.array(h, np.float64), np.array(c, np.float64) + np.array(h, np.float64))
    origin = box((0, 2.0, 0), (4, 1.6, 4))
    p = []
    if name == "dup_flat":
        # 8 primitives, the flat scan, meshes in the LDS arena under default tuning
        head = header(3, "0 2.5 6", "0 0.5 0", False)
        p += twice(("red", "green"), "plane", plane="0 1 0 0")
        p += twice(("blue", "gold"), "sphere", pos="-1.25 0.75 0", radius="0.75")
        p += twice(("white", "red"), "mesh", pos="1.25 0.25 0", rot=ROT_Y, scale="0.75", mesh="pyramid")
        p.append(prim("mesh", "blue", pos="0 0 1.5", scale="1.5", mesh="quad"))
        p.append(prim("mesh", "light", **LIGHT))
        aims = [box((-1.25, 0.75, 0), (0.75, 0.75, 0.75)), box((1.25, 0.8, 0), (0.8, 0.6, 0.8)), box((0, 0, 1.5), (0.75, 0, 0.75)),
                box((0, 0, 0), (3, 0, 3))]
    elif name == "dup_order":
        # ties between primitives whose leaf boxes differ: which of the two the scene walk reaches first depends on the ray
        head = header(3, "0 3 6", "0 0.5 0", False)
        p.append(prim("plane", "grey", plane="0 1 0 0"))
        p.append(prim("mesh", "red", pos="0 0 0", scale="3", mesh="quad"))                       # a quad in the plane
        p.append(prim("mesh", "green", pos="-0.5 1 0", scale="2", mesh="quad"))                  # coplanar quads at y = 1, partly overlapping
        p.append(prim("mesh", "blue", pos="0.5 1 0", scale="2", mesh="quad"))
        p.append(prim("mesh", "gold", pos="0 1 0.5", scale="1", mesh="quad"))
        p.append(prim("mesh", "white", pos="0.25 1 -0.25", scale="1.5", mesh="quad"))
        p.append(prim("mesh", "red", pos="0 1 0", rot=ROT_Y, scale="2", mesh="quad"))
        p.append(prim("sphere", "blue", pos="2 1 -1.5", radius="0.5"))                           # one sphere as radius 0.5 x scale 1 and 0.25 x 2
        p.append(prim("sphere", "gold", pos="2 1 -1.5", scale="2", radius="0.25"))
        p.append(prim("sphere", "green", pos="-2 0.5 1.5", radius="0.5"))                        # spheres that overlap without coinciding
        p.append(prim("sphere", "white", pos="-1.75 0.5 1.5", radius="0.5"))
        p.append(prim("mesh", "light", **LIGHT))
        aims = [box((0, 1, 0), (1.5, 0, 1.2)), box((0, 1, 0), (1.5, 0, 1.2)), box((0, 0, 0), (1.5, 0, 1.5)), box((2, 1, -1.5), (0.5, 0.5, 0.5)),
                box((-2, 0.5, 1.5), (0.5, 0.5, 0.5))]
    elif name == "dup_moving":
        # the duplicates move: equal start and end transforms (translation, rotation, scale), ray time uniform in [0, 1]
        head = header(3, "0 2.5 6.5", "0 0.75 0", True)
        p += twice(("red", "green"), "plane", plane="0 1 0 0")
        p += twice(("blue", "gold"), "sphere", pos="-1.5 0.75 0 , -1 1.25 0.5", scale="1 , 1.5", radius="0.5")
        p += twice(("white", "red"), "mesh", pos="1.25 0.25 0 , 1.5 0.5 -0.5", rot="0 0 0 1 , " + ROT_Y, scale="0.75 , 0.5", mesh="pyramid")
        p += twice(("green", "blue"), "mesh", pos="0 1.5 -1 , 0.5 1.5 -1", rot="0 0 0 1 , " + ROT_Y, scale="1.5", mesh="quad")
        p.append(prim("mesh", "gold", pos="-0.5 0 1.5 , 0.5 0 1.5", scale="1.5", mesh="quad"))  # slides in the plane
        p.append(prim("mesh", "light", **LIGHT))
        aims = [box((-1.25, 1.0, 0.25), (0.9, 0.9, 0.9)), box((1.4, 0.7, -0.25), (0.8, 0.6, 0.8)), box((0.25, 1.5, -1), (1.0, 0, 0.8)),
                box((0, 0, 1.5), (1.2, 0, 0.75)), box((0, 0, 0), (3, 0, 3))]
    elif name == "dup_scene_bvh":
        # 76 primitives, beyond the flat scan's 64: the scene walk.  12 sphere pairs, 6 pyramid pairs, 8 quads in the (doubled) plane that
        # overlap in pairs, single spheres for the rest
        head = header(2, "0 4 8", "0 0.5 0", False)
        p += twice(("grey", "white"), "plane", plane="0 1 0 0")
        mats = [m[0] for m in MATERIALS]
        cells = [(x, z) for z in (-3, -1.5, 0, 1.5, 3) for x in (-3.75, -2.25, -0.75, 0.75, 2.25, 3.75)]      # 30 cells
        k = 0
        for i in range(12):
            x, z = cells[k]; k += 1
            p += twice((mats[i % 6], mats[(i + 1) % 6]), "sphere", pos="%g 0.5 %g" % (x, z), radius="0.5")
            aims.append(box((x, 0.5, z), (0.5, 0.5, 0.5)))
        for i in range(6):
            x, z = cells[k]; k += 1
            p += twice((mats[(i + 2) % 6], mats[(i + 3) % 6]), "mesh", pos="%g 0.125 %g" % (x, z), rot=ROT_Y if i & 1 else None, scale="0.5", mesh="pyramid")
            aims.append(box((x, 0.5, z), (0.5, 0.4, 0.5)))
        for i in range(4):
            x, z = cells[k]; k += 1
            p.append(prim("mesh", mats[i % 6], pos="%g 0 %g" % (x, z), scale="1", mesh="quad"))
            p.append(prim("mesh", mats[(i + 3) % 6], pos="%g 0 %g" % (x + 0.25, z + 0.25), scale="1", mesh="quad"))
            aims.append(box((x + 0.125, 0, z + 0.125), (0.6, 0, 0.6)))
        for i in range(76 - 2 - 24 - 12 - 8 - 1):
            x, z = cells[k % 30]; k += 1
            up = 0.4 if k <= 30 else 1.6
            p.append(prim("sphere", mats[i % 6], pos="%g %g %g" % (x, up, z), radius="0.4"))
        p.append(prim("mesh", "light", pos="0 5 0", rot="1 0 0 0", scale="3", mesh="quad", light=1))
        origin = box((0, 3.0, 0), (5, 2.5, 5))
    elif name == "dup_walked":
        # for k_walk / k_walk_rays under Tuning(walk_min_tris=0, small_mesh_bytes=0): 6 mesh primitives (at most 7 are walked), duplicated
        # instances of one mesh, a walked quad coplanar with a plane
        head = header(3, "0 2.5 6", "0 0.5 0", False)
        p.append(prim("plane", "grey", plane="0 1 0 0"))
        p += twice(("white", "red"), "mesh", pos="-1.25 0.25 0", scale="0.75", mesh="pyramid")
        p += twice(("blue", "gold"), "mesh", pos="1.25 0.25 0", rot=ROT_Y, scale="0.75", mesh="pyramid")
        p.append(prim("mesh", "green", pos="0 0 1.5", scale="2", mesh="quad"))
        p += twice(("green", "blue"), "sphere", pos="0 0.5 -1.5", radius="0.5")
        p.append(prim("mesh", "light", **LIGHT))
        aims = [box((-1.25, 0.8, 0), (0.8, 0.6, 0.8)), box((1.25, 0.8, 0), (0.8, 0.6, 0.8)), box((0, 0, 1.5), (1, 0, 1)),
                box((0, 0.5, -1.5), (0.5, 0.5, 0.5))]
    elif name == "dup_triangles":
        # ties inside one mesh: two faces of the pyramid repeated on vertices of their own -- bit-equal t, other interpolated normals
        head = header(3, "0 2.5 5", "0 0.75 0", False)
        p.append(prim("plane", "grey", plane="0 1 0 0"))
        p.append(prim("mesh", "white", pos="0 0.25 0", rot=ROT_A, scale="1.25", mesh="pyramid2"))
        p.append(prim("mesh", "light", **LIGHT))
        aims = [box((0, 1.0, 0), (0.9, 0.7, 0.9))]
        return head + "\n" + MESHES + "\n" + pyramid_repeated(pyramid2) + "\n" + "\n\n".join(p) + "\n", aims, origin
    else:
        raise KeyError(name)
    return head + "\n" + MESHES + "\n" + "\n\n".join(p) + "\n", aims, origin


# ---------------------------------------------------------------------------------------------------------------------------------
# rays: made again by the tests from the seed, so only Generator.random / integers and float32 arithmetic

def _normalised(d):
    d = d.astype(F)
    s = d[:, 0]*d[:, 0]
    s = s + d[:, 1]*d[:, 1]
    s = s + d[:, 2]*d[:, 2]
    return (d/np.sqrt(s)[:, None]).astype(F)


def _uniform(rng, n, lo, hi):
    return (lo + rng.random((n, 3))*(hi - lo)).astype(F)


def _targets(aims, which, u):
    lo, hi = np.array([a[0] for a in aims])[which], np.array([a[1] for a in aims])[which]
    return (lo + u*(hi - lo)).astype(F)


def _aimed(rng, n, aims, origin):
    o = _uniform(rng, n, *origin)
    which = rng.integers(0, len(aims), n)
    u = rng.random((n, 3))
    return o, _normalised(_targets(aims, which, u) - o)


def first_rays(name, camera_rays, extra=None):
    """The rays that do not depend on a record, as rows origin(3) dir(3) time: aimed into the geometry, axis-aligned (one or two direction
    components exactly 0, not normalised again), the scene's camera rays (pixel corners, time 1 and 0.25), and `extra` (dup_triangles: at the
    mesh's shared edges and vertices)."""
    _, aims, origin = scene_text(name)
    rng = np.random.default_rng(20261019 + SCENES.index(name))
    o, d = _aimed(rng, N_AIMED, aims, origin)
    t = rng.random(N_AIMED).astype(F)
    ao, ad = _aimed(rng, N_AXIS, aims, origin)
    zero = rng.integers(0, 3, N_AXIS)
    ad[np.arange(N_AXIS), zero] = 0.0
    two = rng.random(N_AXIS) < 0.5
    ad[two, (zero[two] + 1) % 3] = 0.0
    ad[(ad == 0).all(axis=1), 1] = -1.0
    at = rng.random(N_AXIS).astype(F)
    cam = np.asarray(camera_rays, F)
    ct = np.where(np.arange(len(cam)) % 2 == 0, F(1.0), F(0.25)).astype(F)
    rows = [np.concatenate([o, d, t[:, None]], axis=1), np.concatenate([ao, ad, at[:, None]], axis=1), np.concatenate([cam, ct[:, None]], axis=1)]
    if extra is not None:
        rows.append(np.asarray(extra, F))
    return np.ascontiguousarray(np.concatenate(rows).astype(F))


def surface_rays(name, first, t_first, hit_first):
    """Rays that start on a previous hit point: o + t d of the first rays that hit (float32, products first), aimed into the geometry again."""
    _, aims, origin = scene_text(name)
    rng = np.random.default_rng(7 + SCENES.index(name))
    src = np.resize(np.nonzero(hit_first)[0], N_SURFACE)
    o = (first[src, 0:3] + (t_first[src, None]*first[src, 3:6]).astype(F)).astype(F)
    which = rng.integers(0, len(aims), N_SURFACE)
    u = rng.random((N_SURFACE, 3))
    d = _normalised(_targets(aims, which, u) - o)
    d[~np.isfinite(d).all(axis=1)] = F(1.0)
    return np.ascontiguousarray(np.concatenate([o, d, first[src, 6:7]], axis=1).astype(F))


def all_rays(name, g):
    """every ray of scene `name` from the corpus file `g` (a mapping) -> rows origin(3) dir(3) time; checks the recorded CRC-32"""
    extra = g[name + "_extra"] if (name + "_extra") in g else None
    first = first_rays(name, g[name + "_camera_rays"], extra)
    prim, t = g[name + "_prim"], g[name + "_t"]
    rows = np.ascontiguousarray(np.concatenate([first, surface_rays(name, first, t[:len(first)], prim[:len(first)] >= 0)]))
    assert zlib.crc32(rows.tobytes()) == int(g[name + "_rays_crc"]), "%s: the rays made from the seed are not the recorded ones" % name
    return rows


def query_rays(rows):
    """rows origin(3) dir(3) time -> the (n, 8) ray layout of trace_rays (origin, time, dir, tmax = inf)"""
    q = np.zeros((len(rows), 8), F)
    q[:, 0:3], q[:, 3], q[:, 4:7], q[:, 7] = rows[:, 0:3], rows[:, 6], rows[:, 3:6], np.inf
    return q


def face_forward(n, d):
    """FaceForward(n, -d) in float32, products summed left to right (maths.h Dot)"""
    n, d = n.astype(F), d.astype(F)
    s = (-d[:, 0])*n[:, 0]
    s = s + (-d[:, 1])*n[:, 1]
    s = s + (-d[:, 2])*n[:, 2]
    return np.where((s < 0)[:, None], -n, n).astype(F)


# ---------------------------------------------------------------------------------------------------------------------------------

def _edge_rays(R, h, prim_index, rng, k=80):
    """dup_triangles: rays aimed exactly at the mesh's shared edges and vertices (world space), as tests/test_gpu_bvh_build._rays builds them"""
    import ctypes as C
    p = R.primitive(h, prim_index)
    g = p.geo.mesh
    pos = np.ctypeslib.as_array(C.cast(g.positions, C.POINTER(C.c_float)), shape=(g.num_vertices, 3)).astype(np.float64)
    idx = np.ctypeslib.as_array(C.cast(g.indices, C.POINTER(C.c_int32)), shape=(g.num_indices//3, 3))
    t = p.start_transform
    q = np.array([t.r.x, t.r.y, t.r.z, t.r.w], np.float64)
    q /= np.linalg.norm(q)
    x, y, z, w = q
    rot = np.array([[1 - 2*(y*y + z*z), 2*(x*y - z*w), 2*(x*z + y*w)], [2*(x*y + z*w), 1 - 2*(x*x + z*z), 2*(y*z - x*w)],
                    [2*(x*z - y*w), 2*(y*z + x*w), 1 - 2*(x*x + y*y)]])
    world = (pos*t.s) @ rot.T + np.array([t.p.x, t.p.y, t.p.z])
    v = world[rng.integers(0, len(world), k)]
    e0, e1 = world[idx[:, 0]], world[idx[:, 1]]
    pick = rng.integers(0, len(e0), k)
    on_edge = e0[pick] + rng.random((k, 1))*(e1[pick] - e0[pick])
    src = np.array([0.0, 2.0, 0.0]) + (rng.random((2*k, 3)) - 0.5)*np.array([8.0, 3.0, 8.0])
    tgt = np.concatenate([v, on_edge])
    d = tgt - src
    o = [src, e0[pick] - (e1[pick] - e0[pick])]
    d = [d/np.linalg.norm(d, axis=1, keepdims=True), e1[pick] - e0[pick]]
    o, d = np.concatenate(o).astype(F), np.concatenate(d).astype(F)
    return np.concatenate([o, d, np.zeros((len(o), 1), F)], axis=1)


def tables(R, h, rows):
    """From the reference's PrimitiveIntersect and PrimitiveBounds alone: accepted t per primitive and ray, [P, n], inf where the primitive
    is not hit, t <= 0, or the ray does not reach its leaf box (the restated slab test of tests/test_gpu_ray_query.py)"""
    from tests.test_gpu_ray_query import _reached
    P = R.num_primitives(h)
    q = query_rays(rows)
    T = np.full((P, len(rows)), np.inf, F)
    for p in range(P):
        hit, t, _ = R.primitive_intersect(h, p, rows)
        reached = _reached(*R.primitive_bounds(h, p), q) if P > 1 else True
        T[p] = np.where((hit != 0) & (t > 0) & reached, t, F(np.inf))
    return T


def stats(T, prim, t):
    """-> dict of masks over the rays, from the tables and Trace()'s records"""
    tmin = T.min(axis=0)
    hit = np.isfinite(tmin)
    assert np.array_equal(hit, prim >= 0) and np.array_equal(t[hit].view(np.uint32), tmin[hit].view(np.uint32)), "Trace() is not the minimum of the tables"
    tied = (T == tmin) & hit
    assert tied[prim[hit], np.nonzero(hit)[0]].all()
    count = tied.sum(axis=0)
    lowest = tied.argmax(axis=0)
    with np.errstate(invalid="ignore"):
        near = (np.isfinite(T) & (T != tmin) & (np.abs(T - tmin) <= F(1e-5)*np.abs(T))).any(axis=0) & hit
    return dict(hit=hit, tied=hit & (count > 1), not_lowest=hit & (count > 1) & (prim != lowest), near=near, sets=tied, count=count)


def make(R, name, tmp):
    def load(text, tag):
        tin = os.path.join(tmp, "%s%s.tin" % (name, tag))
        with open(tin, "w") as fh:
            fh.write(text)
        return R.load_tin(tin)

    h = load(scene_text(name)[0], "")
    pack = os.path.join(tmp, name + ".pack")
    R.write_pack(h, pack)
    cam, opt = R.camera_options(h)
    assert (opt.width, opt.height) == (W, H)
    jj, ii = np.mgrid[0:H, 0:W]
    camera_rays = R.camera_rays(cam, W, H, np.stack([ii.ravel(), jj.ravel()], axis=1).astype(F))
    out = {"pack": np.frombuffer(open(pack, "rb").read(), np.uint8), "camera_rays": camera_rays}
    extra = None
    if name == "dup_triangles":
        extra = out["extra"] = _edge_rays(R, h, 1, np.random.default_rng(5))
    first = first_rays(name, camera_rays, extra)
    prim1, t1, _ = R.trace(h, first)
    rows = np.ascontiguousarray(np.concatenate([first, surface_rays(name, first, t1, prim1 >= 0)]))
    prim, t, nrm = R.trace(h, rows)
    assert np.array_equal(prim[:len(first)], prim1) and np.array_equal(t[:len(first)].view(np.uint32), t1.view(np.uint32))
    T = tables(R, h, rows)
    s = stats(T, prim, t)
    out.update(rays_crc=np.uint32(zlib.crc32(rows.tobytes())), prim=prim.astype(np.int16), t=t, normal=nrm,
               tied_sets=np.packbits(s["sets"].T, axis=1, bitorder="little"))
    line = "%-14s prims %2d  rays %5d  hit %5d  tied %5d  not lowest %5d  near %5d" % (
        name, R.num_primitives(h), len(rows), s["hit"].sum(), s["tied"].sum(), s["not_lowest"].sum(), s["near"].sum())
    # the winner of a tied pair is not a fixed member of it: pairs both of whose members win on some rays
    pairs = {}
    two = np.nonzero(s["tied"] & (s["count"] == 2))[0]
    members = np.stack([s["sets"][:, two].argmax(axis=0), T.shape[0] - 1 - s["sets"][::-1, two].argmax(axis=0)], axis=1) if len(two) else np.zeros((0, 2), int)
    for (a, b), w in zip(members, prim[two]):
        pairs.setdefault((int(a), int(b)), set()).add(int(w))
    both = sorted(k for k, v in pairs.items() if len(v) == 2)
    line += "  pairs with both winners %d" % len(both)
    if name == "dup_triangles":
        # which triangle of a repeated pair gave the normal: the same mesh with the originals only, the repeats only, neither
        aux = {}
        for which in ("originals", "repeats", "neither"):
            ha = load(scene_text(name, which)[0], "_" + which)
            aux[which] = R.primitive_intersect(ha, 1, rows)
            R.free(ha)
        (ha_, ta, na), (hb_, tb, nb), (hc_, tc, _) = aux["originals"], aux["repeats"], aux["neither"]
        mesh_wins = prim == 1
        pair = mesh_wins & (ha_ != 0) & (hb_ != 0) & (ta == t) & (tb == t) & ((hc_ == 0) | (tc > t) | (tc <= 0))
        fa, fb = face_forward(na, rows[:, 3:6]), face_forward(nb, rows[:, 3:6])
        is_a = (fa.view(np.uint32) == nrm.view(np.uint32)).all(axis=1)
        is_b = (fb.view(np.uint32) == nrm.view(np.uint32)).all(axis=1)
        assert (is_a | is_b)[pair].all()
        differ = pair & ~(is_a & is_b)
        # the repeat of the (local) +z face is triangle 0, ahead of its original; the repeat of the -z face is the last triangle, behind its
        # original: the lowest index of a tied pair is the repeat on the +z face and the original on the -z face
        hp = R.primitive(h, 1)
        local_z = _local_z(hp, rows, t)
        plus_z = local_z > 0
        not_lowest = differ & np.where(plus_z, is_a, is_b)
        out["alt_normal"] = np.where(pair[:, None], np.where(is_a[:, None], fb, fa), F(0.0)).astype(F)
        out["pair"] = pair
        # rays on which ANOTHER of the mesh's six triangles has a hit within 1e-5 |t| of the mesh's (equal included: a shared edge or vertex):
        # there the mesh walk's answer rests on its tree -- MeshQuery drops a child whose box entry t is not below the closest t so far
        # (intersection.h:711-714), and of equal hits the first visited stays -- so only the reference's own tree can be held to these bits
        hit_m, t_m, n_m = R.primitive_intersect(h, 1, rows)
        others = np.zeros(len(rows), np.int32)
        for k in range(6):
            hk = load(scene_text(name, "tri%d" % k)[0], "_tri%d" % k)
            ok, tk, _ = R.primitive_intersect(hk, 1, rows)
            R.free(hk)
            with np.errstate(invalid="ignore"):
                others += (ok != 0) & (tk > 0) & (np.abs(tk - t_m) <= F(1e-5)*np.abs(tk))
        contested = (hit_m != 0) & (others > 1)
        assert not (contested & ~(hit_m != 0)).any() and ((others >= 1) | (hit_m == 0) | (t_m <= 0)).all()
        out["contested"] = contested
        out.update(mesh_hit=hit_m.astype(np.uint8), mesh_t=t_m, mesh_normal=n_m)
        line += "\n%-14s inside the mesh: tied %5d  normals differ %5d  not lowest %5d (+z pair %d, -z pair %d)  contested %d (tied and not contested %d)" % (
            "", pair.sum(), differ.sum(), not_lowest.sum(), (not_lowest & plus_z).sum(), (not_lowest & ~plus_z).sum(), contested.sum(), (pair & ~contested).sum())
        assert (pair & ~contested).sum() >= FLOOR_TIED and contested.sum() <= 0.01*pair.sum(), "dup_triangles: too many contested rays: fewer edge rays"
        counts = (int(pair.sum()), int(not_lowest.sum()), int(differ.sum()))
    else:
        counts = (int(s["tied"].sum()), int(s["not_lowest"].sum()), int(s["near"].sum()))
    accum, rad, _ = R.render_seeded(h, cam, opt, 0, PASSES, want_accum=True, want_radiance=True, threads=8)
    assert np.isfinite(rad).all()
    out.update(radiance=rad, accum=accum)
    if name == "dup_flat":
        # Trace() on the beauty's own camera samples (the jittered rays of those passes, in slot order): what the feature buffers hold
        from tests.test_gpu_radiance_query import _starts
        st = _starts(R, cam, W, H, PASSES)
        bp, bt, bn = R.trace(h, np.stack([st[f] for f in ("ox", "oy", "oz", "dx", "dy", "dz", "time")], axis=1))
        out.update(beauty_prim=bp.astype(np.int16), beauty_t=bt, beauty_normal=bn)
    R.free(h)
    print(line, flush=True)
    assert counts[0] >= FLOOR_TIED, "%s: %d exactly tied rays" % (name, counts[0])
    assert counts[1] >= FLOOR_NOT_LOWEST, "%s: %d tied rays whose winner is not the lowest index" % (name, counts[1])
    assert counts[2] >= (FLOOR_NOT_LOWEST if name == "dup_triangles" else FLOOR_NEAR), "%s: %d near ties / differing normals" % (name, counts[2])
    if name == "dup_order":
        assert both, "dup_order: no tied pair both of whose members win"
    return {name + "_" + k: v for k, v in out.items()}


def _local_z(p, rows, t):
    """the local z of the hit point o + t d under the (still) primitive's pose -- float64, only to tell the pyramid's +z face from its -z face"""
    tr = p.start_transform
    q = np.array([tr.r.x, tr.r.y, tr.r.z, tr.r.w], np.float64)
    q /= np.linalg.norm(q)
    x, y, z, w = q
    rot = np.array([[1 - 2*(y*y + z*z), 2*(x*y - z*w), 2*(x*z + y*w)], [2*(x*y + z*w), 1 - 2*(x*x + z*z), 2*(y*z - x*w)],
                    [2*(x*z - y*w), 2*(y*z + x*w), 1 - 2*(x*x + y*y)]])
    with np.errstate(all="ignore"):
        hp = rows[:, 0:3].astype(np.float64) + np.where(np.isfinite(t), t, 0.0)[:, None].astype(np.float64)*rows[:, 3:6]
    return ((hp - np.array([tr.p.x, tr.p.y, tr.p.z])) @ rot)[:, 2]


def main():
    from tests.oracle_api import RefOracle
    R = RefOracle()
    tmp = tempfile.mkdtemp()
    out = {}
    for name in SCENES:
        out.update(make(R, name, tmp))
    # (np.savez stamps the zip entries with the time of day: written through ZipFile with a fixed date, the same bytes every time)
    import zipfile
    path = os.path.join(HERE, "ties.golden.npz")
    with zipfile.ZipFile(path, "w") as z:
        for k in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(2026, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue(), compresslevel=9)
    print("wrote ties.golden.npz (%.1f KB)" % (os.path.getsize(path)/1e3))


if __name__ == "__main__":
    main()

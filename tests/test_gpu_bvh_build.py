"""Device-built mesh BVHs read back node by node (tinsel_hip_mesh_tree) and checked against the host reference (tests/bvh_host.py).

A corpus of meshes is generated at test time (seeded numpy data -> inline `mesh` blocks of a .tin -> the reference's loader -> a pack
in tmp_path) at the sizes and shapes where tree builders go wrong: 2-4 triangles, the edges of the 256-thread blocks, of the 2048-key
sort / scan tiles and of kWalkTopNodes, the first size where k_lbvh_bounds gives a thread two triangles; equal centroids, flat and
line meshes, negative coordinates, one far-away triangle, duplicated triangles, Morton codes that differ at successive bits, and
extents whose PLOC areas overflow.  Renderers are created with small_mesh_bytes=0, so even a 2-triangle mesh lives in HBM and is
rebuilt.  For every mesh and builder: the tree's invariants, then LBVH node for node (boxes bit-equal) and PLOC in canonical form
against the host build; rays through PrimitiveIntersect under all three trees; refits; and the two refusals of set_mesh_bvh."""
import ctypes as C
import os

import numpy as np
import pytest

from tinsel_amd import abi
from tests import bvh_host as bh
from tests import oracle_api as oa

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not oa.have_ref(), reason="oracle/_ref not built (needs the reference sources)")]

F = np.float32
TUNING = dict(small_mesh_bytes=0)

SCENE = """options
{
\twidth 16
\theight 12
\tmaxDepth 2
\tfilter box 0.5 1.0
}

camera
{
\tposition %s
\ttarget %s
\tfov 50
}

sky
{
\thorizon 0.6 0.7 0.8
\tzenith 0.2 0.3 0.9
}

material m0
{
\tcolor 0.7 0.6 0.5
\troughness 0.4
}

mesh corpus
{
\tverts %d
%s

\ttris %d
%s
}

primitive
{
\ttype mesh
\tmesh corpus
\tmaterial m0
}
"""


# ---------------------------------------------------------------------------------------------------------------------------------
# the corpus: (positions [V,3] float32, indices [n,3] int32); every shape is a function of (n, seed)

def _soup(rng, n, centre=(0.0, 0.0, 0.0), size=0.2):
    c = rng.uniform(-1.0, 1.0, (n, 1, 3)) + np.asarray(centre)
    return (c + rng.uniform(-size, size, (n, 3, 3))).astype(F)


def _sym(rng, n):
    """triangles whose boxes are [-e, e] exactly: every box centre is 0, the triangles differ"""
    e = rng.uniform(0.01, 1.0, (n, 3)).astype(F)
    r = rng.uniform(-1.0, 1.0, (n, 3)).astype(F)
    t = np.stack([-e, np.stack([e[:, 0], e[:, 1]*r[:, 0], e[:, 2]], 1), np.stack([e[:, 0]*r[:, 1], e[:, 1], e[:, 2]*r[:, 2]], 1)], 1)
    return t.astype(F)


def _morton_chain(n):
    """tiny triangles centred where the Morton codes have exactly one bit set, bit 0 to bit 29 (the deepest LBVH the codes allow), plus
    one at the origin and one at (1, 1, 1) that fix the extent; the rest repeat the first ones"""
    h = F(2.0**-20)
    cs = [np.zeros(3, F)]
    for p in range(30):
        c = np.zeros(3, F)
        c[2 - p % 3] = F(2.0**(p//3))/F(1024)
        cs.append(c)
    cs.append(np.ones(3, F))
    cs = np.array([cs[k % len(cs)] for k in range(n)], F)
    t = np.stack([cs - h, cs + np.array([h, -h, h], F), cs + h], 1)
    return t.astype(F)


def _grid(rng, n, signed_zero):
    """a flat triangulated grid in z = 0 with SHARED vertices (n triangles: whole quads plus one more); z = +0.0 or -0.0 per vertex"""
    q = (n + 1)//2
    w = max(1, int(np.ceil(np.sqrt(q))))
    h = (q + w - 1)//w
    xs, ys = np.meshgrid(np.arange(w + 1, dtype=F)/F(w), np.arange(h + 1, dtype=F)/F(max(h, 1)))
    zs = np.where(rng.random(xs.shape) < 0.5, F(-0.0), F(0.0)) if signed_zero else np.zeros(xs.shape, F)
    pos = np.stack([xs.ravel(), ys.ravel(), zs.ravel()], 1).astype(F)
    idx = []
    for j in range(h):
        for i in range(w):
            a, b, c, d = j*(w + 1) + i, j*(w + 1) + i + 1, (j + 1)*(w + 1) + i + 1, (j + 1)*(w + 1) + i
            idx += [(a, b, c), (a, c, d)]
    return pos, np.array(idx[:n], np.int32)


def make_mesh(shape, n, seed=0):
    rng = np.random.default_rng([n, seed, sum(map(ord, shape))])
    if shape == "flat":
        return _grid(rng, n, True)
    if shape == "soup":
        t = _soup(rng, n)
    elif shape == "identical":
        t = np.repeat(_soup(rng, 1), n, axis=0)
    elif shape == "same_centroid":
        t = _sym(rng, n)
    elif shape == "line":
        t = np.zeros((n, 3, 3), F)
        t[:, :, 0] = rng.uniform(-1.0, 1.0, (n, 3))
    elif shape == "negative":
        t = _soup(rng, n, centre=(-3.0, -3.0, -3.0))
    elif shape == "far_one":
        t = _soup(rng, n, size=1e-4)
        t[-1] = np.array([[1e6, 1e6, 1e6], [1e6 + 1, 1e6, 1e6], [1e6, 1e6 + 1, 1e6]], F)
    elif shape == "duplicated":
        t = np.repeat(_soup(rng, (n + 1)//2), 2, axis=0)[:n]
    elif shape == "morton_chain":
        t = _morton_chain(n)
    elif shape in ("huge19", "huge30"):
        t = (_soup(rng, n, size=0.5)*F(1e19 if shape == "huge19" else 1e30)).astype(F)
    elif shape == "flat_huge":            # flat boxes wider than FLT_MAX: dz*dx = 0*inf
        t = (_soup(rng, n, size=0.5)*F(1.5e38)).astype(F)
        t[:, :, 2] = 0.0
    elif shape == "nested":
        t = _nested(n)
    else:
        raise KeyError(shape)
    t = np.ascontiguousarray(t, F)
    return t.reshape(-1, 3), np.arange(3*n, dtype=np.int32).reshape(n, 3)


def _nested(n):
    """n triangles with one box centre, each inside the one before it: every PLOC round merges ONE pair at the small end (a chain
    n - 1 deep); the reference's SAH sweep still splits them evenly"""
    e = (F(1.0) - np.arange(n, dtype=F)*F(0.5/n)).astype(F)
    t = np.zeros((n, 3, 3), F)
    t[:, 0] = -e[:, None]
    t[:, 1] = np.stack([e, -e, e], 1)
    t[:, 2] = np.stack([e, e, F(0)*e], 1)
    return t


# shapes whose reference SAH tree is a chain (zero or infinite areas: the sweep's costs are NaN): only small sizes fit the LDS stack
SMALL = (2, 3, 4, 63, 64, 65)
SIZES = {
    "soup": (2, 3, 4, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 2050, 4097, 65537),
    "identical": SMALL, "line": SMALL, "huge19": SMALL, "huge30": SMALL, "flat_huge": SMALL,
    "same_centroid": (2, 3, 4, 64, 257, 2049), "flat": (2, 3, 4, 64, 257, 2049), "negative": (2, 3, 64, 2049),
    "far_one": (3, 64, 2049), "duplicated": (2, 4, 64, 2050), "morton_chain": (32, 63, 257),
}
SHAPES = list(SIZES)
CASES = [(s, n) for s in SHAPES for n in SIZES[s]]
MODES = [(abi.BVH_LBVH, "lbvh"), (abi.BVH_PLOC, "ploc")]


def _f9(x):
    return "%.9g" % x


def write_pack(base, pos, idx):
    """.tin with the mesh inline -> the reference's loader -> base + '.pack'; returns (pack path, RefOracle, handle)"""
    lo, hi = pos.min(axis=0).astype(np.float64), pos.max(axis=0).astype(np.float64)
    mid = 0.5*(lo + hi) if np.all(np.isfinite(0.5*(lo + hi))) else np.zeros(3)
    ext = float(np.max(hi - lo)) if np.all(np.isfinite(hi - lo)) else 1.0
    eye = mid + np.array([0.3, 0.4, 1.0])*max(ext, 1e-3)*2.0
    vt = "\n".join("\t%s %s %s" % tuple(_f9(v) for v in p) for p in pos.astype(np.float64))
    tt = "\n".join("\t%d %d %d" % tuple(t) for t in idx)
    tin = base + ".tin"
    with open(tin, "w") as fh:
        fh.write(SCENE % (" ".join(map(_f9, eye)), " ".join(map(_f9, mid)), len(pos), vt, len(idx), tt))
    R = oa.RefOracle()
    h = R.load_tin(tin)
    R.write_pack(h, base + ".pack")
    return base + ".pack", R, h


def pack_triangles(scene, prim=0):
    """the mesh's triangles [n,3,3] as the pack holds them (its own vertex order), and (positions, indices)"""
    p = C.cast(scene.desc.primitives, C.POINTER(abi.Primitive))[prim]
    g = p.geo.mesh
    pos = np.ctypeslib.as_array(C.cast(g.positions, C.POINTER(C.c_float)), shape=(g.num_vertices, 3)).copy()
    idx = np.ctypeslib.as_array(C.cast(g.indices, C.POINTER(C.c_int32)), shape=(g.num_indices//3, 3)).copy()
    return pos[idx], pos, idx


class Mesh:
    def __init__(self, tmp, shape, n, seed=0):
        import tinsel_amd
        pos, idx = make_mesh(shape, n, seed)
        path, self.R, self.h = write_pack(os.path.join(str(tmp), "%s_%d" % (shape, n)), pos, idx)
        self.scene = tinsel_amd.Scene.load_pack(path)
        self.tris, self.pos, self.idx = pack_triangles(self.scene)
        assert np.array_equal(self.pos.view(np.uint32), pos.view(np.uint32)) and np.array_equal(self.idx, idx)
        self.r = tinsel_amd.create_gpu_renderer(self.scene, 0, abi.Tuning(**TUNING))

    def tree(self):
        return self.r.mesh_tree(0)

    def close(self):
        self.r.close()
        self.R.free(self.h)


def host_build(mode, tris):
    return bh.build_lbvh(tris) if mode == abi.BVH_LBVH else bh.build_ploc(tris)


def check_against_host(m, mode, label):
    nodes, meta = m.tree()
    bh.check_tree(nodes, meta, m.tris, True, m.r.stack_entries)
    want, need, top = host_build(mode, m.tris)
    assert meta["stackNeed"] == need and meta["topCount"] == top
    if mode == abi.BVH_LBVH:
        # deterministic ids: Karras numbering, then the breadth-first renumbering -- node for node
        assert np.array_equal(nodes["left"], want["left"]) and np.array_equal(nodes["right"], want["right"]), label
        for f in ("lmin", "lmax", "rmin", "rmax"):
            assert np.array_equal(bh.box_bits(nodes[f]), bh.box_bits(want[f])), (label, f)
    else:
        assert np.array_equal(bh.canonical(nodes), bh.canonical(want)), label
    return nodes, meta


# ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,n", CASES, ids=["%s-%d" % c for c in CASES])
def test_device_trees_match_host_reference(tmp_path, shape, n):
    m = Mesh(tmp_path, shape, n)
    try:
        ref_nodes, ref_meta = m.tree()
        bh.check_tree(ref_nodes, ref_meta, m.tris, False, m.r.stack_entries)
        assert ref_meta["inArena"] == 0
        for mode, label in MODES:
            m.r.set_mesh_bvh(mode)
            check_against_host(m, mode, "%s %s-%d" % (label, shape, n))
        m.r.set_mesh_bvh(abi.BVH_REFERENCE)
        nodes, meta = m.tree()
        assert meta == ref_meta and nodes.tobytes() == ref_nodes.tobytes()
    finally:
        m.close()


def test_reference_tree_readback_of_an_arena_mesh(tmp_path):
    """a mesh in the LDS-staged arena (default tuning): read from the arena's HBM copy, the same tree as in HBM"""
    import tinsel_amd
    pos, idx = make_mesh("soup", 12)
    path, R, h = write_pack(os.path.join(str(tmp_path), "arena"), pos, idx)
    scene = tinsel_amd.Scene.load_pack(path)
    tris = pack_triangles(scene)[0]
    a = tinsel_amd.create_gpu_renderer(scene, 0, abi.Tuning())
    b = tinsel_amd.create_gpu_renderer(scene, 0, abi.Tuning(**TUNING))
    try:
        na, ma = a.mesh_tree(0)
        nb, mb = b.mesh_tree(0)
        assert ma["inArena"] == 1 and mb["inArena"] == 0
        bh.check_tree(na, ma, tris, False, a.stack_entries)
        assert np.array_equal(bh.canonical(na), bh.canonical(nb))
    finally:
        a.close()
        b.close()
        R.free(h)


# ---------------------------------------------------------------------------------------------------------------------------------
# rays: hit flags and t bit-identical under the three trees, and equal to the reference's PrimitiveIntersect under its own tree

def _rays(m, rng, k=2048):
    lo, hi = m.pos.min(axis=0).astype(np.float64), m.pos.max(axis=0).astype(np.float64)
    mid, ext = 0.5*(lo + hi), np.maximum(hi - lo, 1e-3)
    o, d = [], []
    # random, from a shell around the box towards points inside it
    u = rng.normal(size=(k, 3))
    o.append(mid + u/np.linalg.norm(u, axis=1, keepdims=True)*np.linalg.norm(ext)*1.5)
    d.append(mid + (rng.random((k, 3)) - 0.5)*ext - o[-1])
    # through the mesh's vertices and along its edges (shared in the grid meshes), from above and grazing in the plane
    v = m.pos[rng.integers(0, len(m.pos), k)].astype(np.float64)
    w = m.pos[rng.integers(0, len(m.pos), k)].astype(np.float64)
    e0, e1 = m.pos[m.idx[:, 0]].astype(np.float64), m.pos[m.idx[:, 1]].astype(np.float64)
    pick = rng.integers(0, len(e0), k)
    o += [v + np.array([0.0, 0.0, 1.0])*ext.max(), e0[pick] - (e1[pick] - e0[pick]), v - (w - v)]
    d += [np.tile([0.0, 0.0, -1.0], (k, 1)), e1[pick] - e0[pick], w - v]
    # axis-aligned (zero direction components), in the plane z = 0 and across it
    ax = np.eye(3)[rng.integers(0, 3, k)]*rng.choice([-1.0, 1.0], (k, 1))
    p = lo + rng.random((k, 3))*(hi - lo)
    o += [p - ax*ext.max()*2.0, np.concatenate([p[:, :2] - ext[:2]*2.0, np.zeros((k, 1))], 1)]
    d += [ax, np.concatenate([rng.normal(size=(k, 2)), np.zeros((k, 1))], 1)]
    # at the corners and face centres of the root box, and from inside it
    corners = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)] + [[0.5, 0.5, 0], [0.5, 0.5, 1], [0.5, 0, 0.5],
                                                                                       [0.5, 1, 0.5], [0, 0.5, 0.5], [1, 0.5, 0.5]], np.float64)
    c = lo + corners[rng.integers(0, len(corners), k)]*(hi - lo)
    src = mid + rng.normal(size=(k, 3))*ext*2.0
    o += [src, lo + rng.random((k, 3))*(hi - lo)]
    d += [c - src, rng.normal(size=(k, 3))]
    o, d = np.concatenate(o), np.concatenate(d)
    with np.errstate(all="ignore"):
        o, d = o.astype(F), d.astype(F)
    ok = np.all(np.isfinite(o), axis=1) & np.all(np.isfinite(d), axis=1) & np.any(d != 0, axis=1)
    return np.concatenate([o[ok], d[ok], np.zeros((ok.sum(), 1), F)], axis=1)


RAY_CASES = [("soup", 257), ("soup", 4097), ("flat", 64), ("flat", 2049), ("duplicated", 64), ("duplicated", 2050), ("identical", 64),
             ("same_centroid", 257), ("line", 65), ("far_one", 2049), ("morton_chain", 257), ("negative", 64), ("huge30", 63),
             ("flat_huge", 64), ("soup", 2), ("flat", 3)]


@pytest.mark.parametrize("shape,n", RAY_CASES, ids=["%s-%d" % c for c in RAY_CASES])
def test_rays_identical_under_all_three_trees(tmp_path, shape, n):
    m = Mesh(tmp_path, shape, n)
    try:
        rows = _rays(m, np.random.default_rng(n))
        out = {}
        for mode, label in MODES + [(abi.BVH_REFERENCE, "reference")]:
            m.r.set_mesh_bvh(mode)
            out[label] = m.r.leaf(4, 0, len(rows), 5, rows=rows)
        hit = out["reference"][:, 0] > 0.5
        # the reference's own traversal keeps a 32-entry stack (intersection.h): its chains over degenerate meshes overflow it, so it is
        # asked only where its tree fits
        if m.tree()[1]["stackNeed"] <= 32:
            want_hit, want_t, want_n = m.R.primitive_intersect(m.h, 0, rows)
            assert np.array_equal(hit, want_hit != 0)
            assert np.array_equal(out["reference"][hit, 1].view(np.uint32), want_t[hit].view(np.uint32))
            # ... and the normal: of two triangles with the same t (shared edges, duplicated triangles) only the visit order names the winner
            differ = (np.ascontiguousarray(out["reference"][hit, 2:5]).view(np.uint32) != np.ascontiguousarray(want_n[hit]).view(np.uint32)).any(axis=1)
            print("%s-%d: %d of %d normals differ from the reference's" % (shape, n, differ.sum(), hit.sum()))
            assert not differ.any()
        print("%s-%d: %d rays, %d hits" % (shape, n, len(rows), hit.sum()))
        for label in ("lbvh", "ploc"):
            assert np.array_equal(out[label][:, 0] > 0.5, hit), label
            # t bit-identical, except where two triangles' t lie within the rounding of the box test: the traversal drops a child whose
            # box entry t is not below the closest t so far (intersection.h), and which triangle survives that depends on the tree
            a, b = out[label][hit, 1].view(np.int32).astype(np.int64), out["reference"][hit, 1].view(np.int32).astype(np.int64)
            moved = a != b
            print("  %s: t differs on %d of %d hits (max %d ulp)" % (label, moved.sum(), hit.sum(), np.abs(a - b).max(initial=0)))
            assert np.abs(a - b).max(initial=0) <= 4 and moved.sum() <= max(2, hit.sum()//100), label
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# refit: the shape stays, the boxes follow the new vertices bit for bit -- under every tree, and the reference tree is kept refitted

def _displacements(m, rng):
    lo, hi = m.pos.min(axis=0), m.pos.max(axis=0)
    inside = (lo + (m.pos - lo)*F(0.5) + (hi - lo)*F(0.25)).astype(F)                # shrinks into the old root box
    leave = (m.pos + rng.normal(size=m.pos.shape).astype(F)*(hi - lo)*F(0.7)).astype(F)  # leaves it
    collapse = m.pos.copy()
    gone = rng.random(len(m.idx)) < 0.3                                                 # triangles collapsed to a point
    collapse[m.idx[gone].ravel()] = m.pos[m.idx[gone, 0]].repeat(3, axis=0)
    return [("inside", inside), ("leave", leave), ("collapse", collapse)]


@pytest.mark.parametrize("mode,label", [(abi.BVH_REFERENCE, "reference")] + MODES, ids=["reference", "lbvh", "ploc"])
@pytest.mark.parametrize("shape,n", [("soup", 65), ("soup", 2049), ("flat", 257)], ids=["soup-65", "soup-2049", "flat-257"])
def test_refit_keeps_shape_and_fits_boxes(tmp_path, mode, label, shape, n):
    m = Mesh(tmp_path, shape, n)
    try:
        m.r.set_mesh_bvh(mode)
        before, meta0 = m.tree()
        for what, pos in _displacements(m, np.random.default_rng(7)):
            m.r.refit_mesh(0, pos)
            nodes, meta = m.tree()
            assert meta == meta0, what
            assert np.array_equal(nodes["left"], before["left"]) and np.array_equal(nodes["right"], before["right"]), what
            bh.check_tree(nodes, meta, pos[m.idx], mode != abi.BVH_REFERENCE, m.r.stack_entries)
        if mode != abi.BVH_REFERENCE:
            m.r.set_mesh_bvh(abi.BVH_REFERENCE)
            ref_nodes, ref_meta = m.tree()
            bh.check_tree(ref_nodes, ref_meta, pos[m.idx], False, m.r.stack_entries)
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals: too deep for the LDS stack; too many PLOC rounds.  Nothing changes, and a render stays bit-identical to the reference

def _render(m):
    cam, opt = m.R.camera_options(m.h)
    m.r.init(opt.width, opt.height)
    m.r.set_pass_index(0)
    return m.r.render(cam, opt, passes=1), cam, opt


@pytest.mark.parametrize("n,why", [(200, "too deep"), (4100, "no progress")], ids=["deep", "rounds"])
def test_refused_ploc_build_changes_nothing(tmp_path, n, why):
    from tinsel_amd.renderer import TinselHipError
    m = Mesh(tmp_path, "nested", n)
    try:
        want = bh.build_lbvh(m.tris)
        if why == "too deep":
            assert bh.build_ploc(m.tris)[1] == n            # the host build: a chain, n - 1 internal levels
        for start in (abi.BVH_REFERENCE, abi.BVH_LBVH):
            m.r.set_mesh_bvh(start)
            nodes0, meta0 = m.tree()
            if start == abi.BVH_LBVH:
                assert meta0["stackNeed"] == want[1]
            stack0 = m.r.stack_entries
            img0, cam, opt = _render(m)
            with pytest.raises(TinselHipError):
                m.r.set_mesh_bvh(abi.BVH_PLOC)
            nodes, meta = m.tree()
            assert meta == meta0 and nodes.tobytes() == nodes0.tobytes() and m.r.stack_entries == stack0
            img, _, _ = _render(m)
            assert np.array_equal(img, img0)
            if start == abi.BVH_REFERENCE:
                ref, _, _ = m.R.render_seeded(m.h, cam, opt, 0, 1)
                assert np.array_equal(img, ref)
    finally:
        m.close()


def test_huge_extents_build_under_ploc(tmp_path):
    """every PLOC area of these meshes is inf (or 0*inf): each cluster still picks a neighbour, the build completes and matches the host"""
    for shape in ("huge30", "flat_huge"):
        m = Mesh(tmp_path, shape, 64)
        try:
            boxes = np.concatenate(bh.tri_boxes(m.tris), 1)
            assert np.all(bh.ploc_area(boxes[:-1], boxes[1:]) == np.inf)
            m.r.set_mesh_bvh(abi.BVH_PLOC)
            check_against_host(m, abi.BVH_PLOC, shape)
        finally:
            m.close()

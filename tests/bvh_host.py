"""Plain host reference of the device mesh-BVH builders (tn_lbvh.h, tn_host_bvh_build.h) and an invariant checker for any tree read
back with tinsel_hip_mesh_tree (numpy, fp32; no GPU).

The library is compiled with -ffp-contract=off, so every fp32 expression below rounds exactly as the kernels' do:
  morton_keys   k_lbvh_bounds + k_lbvh_keys + the stable sort: ordered-uint min / max of the box centres 0.5f*(lo + hi),
                (c - mn)/ext (0 where ext is 0), *1024 clamped to [0, 1023], 10-bit expansion, key = code << 32 | index
  build_lbvh    the binary radix tree over the unique keys, split top-down at the highest differing bit (for unique keys this is
                the tree of Karras' construction), numbered as Karras numbers it, then the breadth-first renumbering of its top
  build_ploc    PLOC round by round (radius 8, area dx*dy + dy*dz + dz*dx, lowest index wins ties, non-finite areas count as +inf,
                mutual pairs merge, order-preserving compaction).  Its internal ids come from an atomicSub on the device: compare PLOC
                trees with `canonical`, not by id.
Trees are Node64 arrays as tinsel_hip_mesh_tree returns them (renderer.HipRenderer.mesh_tree): structured arrays with fields lmin,
lmax, rmin, rmax [.,3] float32 and left, right uint32 (bit 31: a leaf; low bits: its triangle)."""
import numpy as np

F = np.float32
LEAF = 0x80000000
PLOC_RADIUS = 8
WALK_TOP_NODES = 2048           # kWalkTopNodes (tn_host_layout.h)
PLOC_MAX_ROUNDS = 4096          # build_device_bvh's guard
NODE_DTYPE = np.dtype([("lmin", "<f4", 3), ("lmax", "<f4", 3), ("rmin", "<f4", 3), ("rmax", "<f4", 3),
                       ("left", "<u4"), ("right", "<u4"), ("pad", "<u4", 2)])


class NoProgress(RuntimeError):
    """PLOC stopped before one cluster was left (the device build refuses the same way)"""


# ---------------------------------------------------------------------------------------------------------------------------------
# boxes and keys

def tri_boxes(tris):
    """tris [n,3,3] float32 (vertices a, b, c) -> (lo [n,3], hi [n,3]): min / max of the three vertices"""
    tris = np.asarray(tris, F)
    a, b, c = tris[:, 0], tris[:, 1], tris[:, 2]
    return np.minimum(a, np.minimum(b, c)), np.maximum(a, np.maximum(b, c))


def float_ordered(f):
    u = np.asarray(f, F).view(np.uint32)
    return np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)


def ordered_float(u):
    u = np.asarray(u, np.uint32)
    return np.where(u & 0x80000000, u & 0x7fffffff, ~u).astype(np.uint32).view(F)


def expand_bits10(v):
    v = np.asarray(v, np.uint64)
    m = np.uint64(0xffffffff)
    v = (v*np.uint64(0x00010001)) & m & np.uint64(0xFF0000FF)
    v = (v*np.uint64(0x00000101)) & m & np.uint64(0x0F00F00F)
    v = (v*np.uint64(0x00000011)) & m & np.uint64(0xC30C30C3)
    v = (v*np.uint64(0x00000005)) & m & np.uint64(0x49249249)
    return v


def morton_codes(tris):
    """the 30-bit Morton code of every triangle's box centre, as k_lbvh_keys computes it"""
    lo, hi = tri_boxes(tris)
    with np.errstate(over="ignore"):
        c = F(0.5)*(lo + hi)
    oc = float_ordered(c)
    mn, mx = ordered_float(oc.min(axis=0)), ordered_float(oc.max(axis=0))
    code = np.zeros(len(c), np.uint64)
    with np.errstate(all="ignore"):
        for k in range(3):
            ext = F(mx[k] - mn[k])
            u = (c[:, k] - mn[k])/ext if ext > F(0) else np.zeros(len(c), F)
            u = np.fmin(np.fmax(u*F(1024), F(0)), F(1023)).astype(F)
            code |= expand_bits10(u.astype(np.uint32)) << np.uint64(2 - k)
    return code


def morton_keys(tris):
    """sorted keys code << 32 | triangle index (unique; the device sorts stably by the code)"""
    keys = (morton_codes(tris) << np.uint64(32)) | np.arange(len(tris), dtype=np.uint64)
    return keys[np.argsort(keys, kind="stable")]


def _high_bit(x):
    """index of the highest set bit of every (nonzero) uint64"""
    x = np.asarray(x, np.uint64)
    b = np.zeros(x.shape, np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        up = (x >> (b + s).astype(np.uint64)) != 0
        b = np.where(up, b + s, b)
    return b


# ---------------------------------------------------------------------------------------------------------------------------------
# trees: children [n-1, 2] int64 over node ids (internal 0..n-2, leaf of sorted position j = n-1+j), the triangle of every leaf id

def lbvh_children(keys):
    """radix tree over sorted unique keys, top-down: a range [lo, hi] splits after the last key whose highest differing bit is clear.
    Karras numbering: an internal node is named by the end of its range that its parent's split touches (root: 0)."""
    n = len(keys)
    children = np.zeros((max(n - 1, 0), 2), np.int64)
    if n < 2:
        return children
    keys = np.asarray(keys, np.uint64)
    lo, hi, ids = np.array([0]), np.array([n - 1]), np.array([0])
    while len(lo):
        b = _high_bit(keys[lo] ^ keys[hi])
        prefix = ((keys[lo] >> b.astype(np.uint64)) | np.uint64(1)) << b.astype(np.uint64)
        gamma = np.searchsorted(keys, prefix, side="left") - 1
        left = np.where(gamma == lo, n - 1 + gamma, gamma)
        right = np.where(gamma + 1 == hi, n - 1 + gamma + 1, gamma + 1)
        children[ids, 0], children[ids, 1] = left, right
        li, ri = gamma > lo, gamma + 1 < hi
        lo, hi, ids = (np.concatenate([lo[li], (gamma + 1)[ri]]), np.concatenate([gamma[li], hi[ri]]),
                       np.concatenate([gamma[li], (gamma + 1)[ri]]))
    return children


def _union(a, b):
    return np.concatenate([np.minimum(a[..., :3], b[..., :3]), np.maximum(a[..., 3:], b[..., 3:])], axis=-1)


def ploc_area(a, b):
    """tn_lbvh.h ploc_area in fp32, non-finite -> +inf"""
    u = _union(a, b)
    with np.errstate(all="ignore"):
        dx, dy, dz = (u[..., 3] - u[..., 0]), (u[..., 4] - u[..., 1]), (u[..., 5] - u[..., 2])
        a = dx*dy + dy*dz + dz*dx
    return np.where(np.isnan(a), F(np.inf), a).astype(F)


def ploc_children(keys, tris, max_rounds=PLOC_MAX_ROUNDS):
    """PLOC over the Morton order; internal ids n-2, n-3, ... in the order the merges are made (ascending cluster position within a
    round -- the device's atomicSub order is not fixed, which `canonical` forgives).  Raises NoProgress like the device build."""
    n = len(keys)
    lo, hi = tri_boxes(tris)
    boxes = np.zeros((2*n - 1, 6), F)
    boxes[n - 1:] = np.concatenate([lo, hi], axis=1)[(keys & np.uint64(0xffffffff)).astype(np.int64)]
    children = np.zeros((max(n - 1, 0), 2), np.int64)
    clusters = np.arange(n - 1, 2*n - 1)
    next_id, rounds = n - 2, 0
    offs = [o for o in range(-PLOC_RADIUS, PLOC_RADIUS + 1) if o]
    while len(clusters) > 1:
        rounds += 1
        if rounds > max_rounds:
            raise NoProgress("more than %d rounds" % max_rounds)
        c = len(clusters)
        i = np.arange(c)
        area = np.full((c, len(offs)), np.inf)                     # outside the array: never chosen
        for q, o in enumerate(offs):
            j = i + o
            ok = (j >= 0) & (j < c)
            a = ploc_area(boxes[clusters[ok]], boxes[clusters[j[ok]]]).astype(np.float64)
            area[ok, q] = np.where(np.isinf(a), 1e300, a)           # an infinite area still beats no neighbour
        nn = i + np.array(offs)[np.argmin(area, axis=1)]           # first least area in ascending j: the lowest index wins ties
        mutual = nn[nn] == i
        make = np.nonzero(mutual & (i < nn))[0]
        if not len(make):
            raise NoProgress("no mutual pair")
        ids = next_id - np.arange(len(make))
        next_id -= len(make)
        a, b = clusters[make], clusters[nn[make]]
        children[ids, 0], children[ids, 1] = a, b
        boxes[ids] = _union(boxes[a], boxes[b])
        clusters = clusters.copy()
        clusters[make] = ids
        clusters = clusters[~(mutual & (i > nn))]
    return children


def bfs_order(children, n, limit=None):
    """internal node ids breadth-first from the root 0, left before right (the first `limit`)"""
    out, frontier = [], [0] if n >= 2 else []
    head = 0
    while head < len(frontier) and (limit is None or len(out) < limit):
        k = frontier[head]
        head += 1
        out.append(k)
        for ch in children[k]:
            if ch < n - 1:
                frontier.append(int(ch))
    return out


def emit(children, keys, tris):
    """the Node64 array the device emits for this tree: boxes fitted exactly, the top min(n-1, 2048) nodes renumbered breadth-first
    (k_bfs_mark / k_bfs_perm / k_lbvh_emit_perm), the rest after them in their old order.  Returns (nodes, stackNeed, topCount)."""
    n = len(keys)
    lo, hi = tri_boxes(tris)
    tri_of = (keys & np.uint64(0xffffffff)).astype(np.int64)
    box = np.zeros((2*n - 1, 6), F)
    box[n - 1:] = np.concatenate([lo, hi], axis=1)[tri_of]
    height = np.zeros(2*n - 1, np.int64)
    for k in reversed(_preorder(children, n)):
        l, r = children[k]
        box[k] = _union(box[l], box[r])
        height[k] = 1 + max(height[l], height[r])
    top = bfs_order(children, n, WALK_TOP_NODES)
    is_top = np.zeros(n - 1, bool)
    is_top[top] = True
    perm = np.empty(n - 1, np.int64)
    perm[top] = np.arange(len(top))
    rest = np.nonzero(~is_top)[0]
    perm[rest] = len(top) + np.arange(len(rest))
    nodes = np.zeros(n - 1, NODE_DTYPE)

    def ref(ch):
        return np.where(ch >= n - 1, LEAF | tri_of[np.clip(ch - (n - 1), 0, n - 1)], perm[np.clip(ch, 0, n - 2)]).astype(np.uint32)

    l, r = children[:, 0], children[:, 1]
    nodes["lmin"][perm], nodes["lmax"][perm] = box[l, :3], box[l, 3:]
    nodes["rmin"][perm], nodes["rmax"][perm] = box[r, :3], box[r, 3:]
    nodes["left"][perm], nodes["right"][perm] = ref(l), ref(r)
    return nodes, int(height[0]) + 1, len(top)


def _preorder(children, n):
    out, stack = [], [0] if n >= 2 else []
    while stack:
        k = stack.pop()
        out.append(k)
        for ch in children[k][::-1]:
            if ch < n - 1:
                stack.append(int(ch))
    return out


def build_lbvh(tris):
    keys = morton_keys(tris)
    return emit(lbvh_children(keys), keys, tris)


def build_ploc(tris):
    keys = morton_keys(tris)
    return emit(ploc_children(keys, tris), keys, tris)


# ---------------------------------------------------------------------------------------------------------------------------------
# comparison and invariants

def box_bits(x):
    """the bits of fp32 boxes with -0 taken as +0 (min / max of +0 and -0 may give either)"""
    return (np.asarray(x, F) + F(0)).view(np.uint32)


def canonical(nodes, root=0):
    """the tree with its internal nodes renumbered in preorder (left first): two trees are the same tree over the same triangles, with
    the same boxes, iff their canonical arrays are equal.  Returns a uint32 array [m, 14]: child refs, then the 12 box words."""
    m = len(nodes)
    if m == 0:
        return np.zeros((0, 14), np.uint32)
    order = []
    stack = [int(root)]
    seen = np.zeros(m, bool)
    while stack:
        k = stack.pop()
        if seen[k]:
            raise AssertionError("node %d reached twice" % k)
        seen[k] = True
        order.append(k)
        for ch in (nodes["right"][k], nodes["left"][k]):
            if not ch & LEAF:
                stack.append(int(ch))
    order = np.array(order)
    new = np.full(m, -1, np.int64)
    new[order] = np.arange(len(order))
    sub = nodes[order]
    refs = []
    for f in ("left", "right"):
        v = sub[f].astype(np.int64)
        leaf = (v & LEAF) != 0
        refs.append(np.where(leaf, v, new[np.where(leaf, 0, v)]).astype(np.uint32))
    bx = np.concatenate([sub["lmin"], sub["lmax"], sub["rmin"], sub["rmax"]], axis=1)
    return np.concatenate([np.stack(refs, axis=1), box_bits(bx)], axis=1)


def check_tree(nodes, meta, tris, device_built, stack_entries=None):
    """Invariants of a mesh tree as the kernels read it; raises AssertionError.  tris [n,3,3]: the mesh's triangles in the pack's
    vertex order.  Returns the maximum leaf depth (root's children: depth 1)."""
    n = len(tris)
    m = len(nodes)
    assert meta["numTris"] == n and meta["numInternal"] == m
    if n == 1:
        assert m == 0 and meta["root"] == LEAF
        return 0
    assert m == n - 1, "%d internal nodes over %d triangles" % (m, n)
    root = meta["root"]
    assert root == 0, "root ref %#x" % root
    refs = np.concatenate([nodes["left"], nodes["right"]]).astype(np.int64)
    leaf = (refs & LEAF) != 0
    tri_ids = refs[leaf] & 0x7fffffff
    assert np.array_equal(np.sort(tri_ids), np.arange(n)), "triangles missing or repeated among the leaves"
    inner = refs[~leaf]
    assert inner.size == 0 or (inner.min() >= 0 and inner.max() < m), "internal ref out of range"
    parents = np.bincount(inner, minlength=m)
    assert parents[0] == 0, "the root has a parent"
    assert np.all(parents[1:] == 1), "internal nodes with %s parents" % sorted(set(parents[1:].tolist()) - {1})
    # breadth-first walk: every node reached once (no cycles), depths, the breadth-first prefix
    lo, hi = tri_boxes(tris)
    depth = np.zeros(m, np.int64)
    order, head = [0], 0
    while head < len(order):
        k = order[head]
        head += 1
        for ch in (nodes["left"][k], nodes["right"][k]):
            if not ch & LEAF:
                depth[ch] = depth[k] + 1
                order.append(int(ch))
    assert len(order) == m, "the walk from the root reaches %d of %d nodes" % (len(order), m)
    leaf_depth = int(depth[np.concatenate([np.nonzero(nodes["left"] & LEAF)[0], np.nonzero(nodes["right"] & LEAF)[0]])].max()) + 1
    # boxes: every child box is the min / max of its subtree's triangles, bit for bit
    sub = np.zeros((m, 6), F)
    for k in reversed(order):
        b = []
        for f, side in (("left", "l"), ("right", "r")):
            ch = int(nodes[f][k])
            want = np.concatenate([lo[ch & 0x7fffffff], hi[ch & 0x7fffffff]]) if ch & LEAF else sub[ch]
            got = np.concatenate([nodes[side + "min"][k], nodes[side + "max"][k]])
            assert np.array_equal(box_bits(got), box_bits(want)), "node %d %s box %s, subtree %s" % (k, f, got, want)
            b.append(want)
        sub[k] = _union(b[0], b[1])
    if device_built:
        assert meta["stackNeed"] == leaf_depth + 1, "stackNeed %d, deepest leaf %d" % (meta["stackNeed"], leaf_depth)
        assert meta["topCount"] == min(m, WALK_TOP_NODES)
    else:
        assert meta["stackNeed"] >= leaf_depth + 1, "stackNeed %d, deepest leaf %d" % (meta["stackNeed"], leaf_depth)
    top = meta["topCount"]
    assert 0 <= top <= m and order[:top] == list(range(top)), "ids [0, %d) are not the breadth-first top" % top
    if stack_entries is not None:
        assert stack_entries >= meta["stackNeed"] + 1, "stack %d entries for a mesh that needs %d" % (stack_entries, meta["stackNeed"])
    return leaf_depth

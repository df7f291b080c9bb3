"""CPU tests of the host reference of the device mesh-BVH builders (tests/bvh_host.py) against brute-force definitions on hand-made
inputs: what tests/test_gpu_bvh_build.py holds the device trees to must itself be right."""
import numpy as np
import pytest

from tests import bvh_host as bh

F = np.float32


def _expand_slow(v):
    return sum(((v >> i) & 1) << (3*i) for i in range(10))


def test_expand_bits10_spreads_every_bit():
    v = np.arange(1024)
    assert np.array_equal(bh.expand_bits10(v), np.array([_expand_slow(int(x)) for x in v], np.uint64))


def test_ordered_uint_round_trips_and_orders():
    f = np.array([-np.inf, -3e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 3e38, np.inf], F)
    u = bh.float_ordered(f)
    assert np.all(np.diff(u.astype(np.int64)) > 0)
    assert np.array_equal(bh.ordered_float(u).view(np.uint32), f.view(np.uint32))


def _tri_at(c, h=F(2.0**-12)):
    c = np.asarray(c, F)
    return np.stack([c - h, c + np.array([h, -h, h], F), c + h]).astype(F)


def test_morton_codes_by_hand():
    # centres at the corners of the unit cube: cell 0 or 1023 on each axis, x the highest bit of every triple
    t = np.stack([_tri_at(c) for c in ([0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1], [0.5, 0.5, 0.5])])
    codes = bh.morton_codes(t)
    full = _expand_slow(1023)
    assert list(codes[:5]) == [0, full << 2, full << 1, full, full*7]
    assert codes[5] == _expand_slow(512)*7
    # extent 0 on every axis: every code is 0; keys fall back to the triangle index
    same = np.stack([_tri_at([0.3, -2.0, 5.0])]*5)
    assert np.all(bh.morton_codes(same) == 0)
    assert np.array_equal(bh.morton_keys(same[::-1]) & np.uint64(0xffffffff), np.arange(5, dtype=np.uint64))


def test_morton_keys_of_negative_and_signed_zero_centres():
    t = np.stack([_tri_at([-4.0, -0.0, -1.0]), _tri_at([-2.0, 0.0, -3.0])])
    t[0, :, 1] = F(-0.0)
    t[1, :, 1] = F(0.0)
    codes = bh.morton_codes(t)
    # x: -4 -> cell 0, -2 -> 1023; y: -0 and +0 differ as ordered uints but their extent is 0; z: -1 -> 1023, -3 -> 0
    assert codes[0] == _expand_slow(1023) and codes[1] == _expand_slow(1023) << 2


def _radix_tree_slow(keys, lo, hi):
    """nested tuples of sorted positions, by the definition: split where the highest differing bit of the range turns on"""
    if lo == hi:
        return lo
    b = int(keys[lo] ^ keys[hi]).bit_length() - 1
    g = max(k for k in range(lo, hi + 1) if not (int(keys[k]) >> b) & 1)
    return (_radix_tree_slow(keys, lo, g), _radix_tree_slow(keys, g + 1, hi))


def _karras_slow(keys):
    """Karras 2012, Algorithm 1, one node at a time in plain Python (the kernel's formulas) -> children by node id"""
    n = len(keys)

    def delta(i, j):
        return -1 if j < 0 or j >= n else 64 - int(keys[i] ^ keys[j]).bit_length()

    out = {}
    for i in range(n - 1):
        d = 1 if delta(i, i + 1) - delta(i, i - 1) >= 0 else -1
        dmin = delta(i, i - d)
        lmax = 2
        while delta(i, i + lmax*d) > dmin:
            lmax *= 2
        l, t = 0, lmax//2
        while t >= 1:
            if delta(i, i + (l + t)*d) > dmin:
                l += t
            t //= 2
        j = i + l*d
        dn, s, t = delta(i, j), 0, l
        while True:
            t = (t + 1)//2
            if delta(i, i + (s + t)*d) > dn:
                s += t
            if t <= 1:
                break
        g = i + s*d + min(d, 0)
        out[i] = (n - 1 + g if min(i, j) == g else g, n - 1 + g + 1 if max(i, j) == g + 1 else g + 1)
    return out


def _nest(children, n, k=0):
    return k - (n - 1) if k >= n - 1 else (_nest(children, n, children[k][0]), _nest(children, n, children[k][1]))


@pytest.mark.parametrize("seed", range(6))
def test_lbvh_children_is_the_radix_tree_and_karras_tree(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 300))
    bits = int(rng.integers(1, 31))           # few code bits: many equal codes, the index decides
    codes = rng.integers(0, 1 << bits, n).astype(np.uint64)
    keys = np.sort((codes << np.uint64(32)) | np.arange(n, dtype=np.uint64))
    ch = bh.lbvh_children(keys)
    assert _nest(ch, n) == _radix_tree_slow(keys, 0, n - 1)
    kar = _karras_slow(keys)
    assert all(tuple(ch[i]) == kar[i] for i in range(n - 1))


def _ploc_slow(keys, tris, radius=bh.PLOC_RADIUS):
    """PLOC by the letter: plain loops, float32 scalars -> nested tuples of triangle ids"""
    lo, hi = bh.tri_boxes(tris)
    tri = [int(k & np.uint64(0xffffffff)) for k in keys]
    cl = [(t, np.concatenate([lo[t], hi[t]]).astype(F)) for t in tri]
    while len(cl) > 1:
        nn = []
        for i in range(len(cl)):
            best, bj = None, -1
            for j in range(max(0, i - radius), min(len(cl), i + radius + 1)):
                if j == i:
                    continue
                a, b = cl[i][1], cl[j][1]
                d = [F(max(a[3 + q], b[3 + q])) - F(min(a[q], b[q])) for q in range(3)]
                with np.errstate(all="ignore"):
                    area = F(F(F(d[0]*d[1]) + F(d[1]*d[2])) + F(d[2]*d[0]))
                area = F(np.inf) if np.isnan(area) else area
                if bj < 0 or area < best:
                    best, bj = area, j
            nn.append(bj)
        out = []
        for i in range(len(cl)):
            j = nn[i]
            if nn[j] == i:
                if i < j:
                    a, b = cl[i][1], cl[j][1]
                    out.append(((cl[i][0], cl[j][0]), np.concatenate([np.minimum(a[:3], b[:3]), np.maximum(a[3:], b[3:])])))
            else:
                out.append(cl[i])
        assert len(out) < len(cl)
        cl = out
    return cl[0][0]


def _ploc_nest(children, keys, n, k=0):
    if k >= n - 1:
        return int(keys[k - (n - 1)] & np.uint64(0xffffffff))
    return (_ploc_nest(children, keys, n, children[k][0]), _ploc_nest(children, keys, n, children[k][1]))


@pytest.mark.parametrize("kind", ["soup", "grid", "identical", "huge", "flat_huge"])
def test_ploc_children_follow_the_rounds_by_the_letter(kind):
    rng = np.random.default_rng(3)
    n = 70
    if kind == "soup":
        t = (rng.uniform(-1, 1, (n, 1, 3)) + rng.uniform(-0.1, 0.1, (n, 3, 3))).astype(F)
    elif kind == "grid":                      # equal areas everywhere: the tie rule decides
        c = np.stack(np.meshgrid(np.arange(7), np.arange(10), [0]), -1).reshape(-1, 3).astype(F)
        t = np.stack([c, c + F([0.5, 0, 0]), c + F([0, 0.5, 0])], 1).astype(F)
    elif kind == "identical":
        t = np.repeat(rng.uniform(-1, 1, (1, 3, 3)).astype(F), n, axis=0)
    elif kind == "huge":                      # every area overflows to inf
        t = (rng.uniform(-1, 1, (n, 3, 3))*1e30).astype(F)
    else:                                     # boxes wider than FLT_MAX in a plane: 0*inf
        t = (rng.uniform(-1, 1, (n, 3, 3))*1.5e38).astype(F)
        t[:, :, 2] = 0
    keys = bh.morton_keys(t)
    ch = bh.ploc_children(keys, t)
    assert _ploc_nest(ch, keys, n) == _ploc_slow(keys, t)


def test_ploc_nested_triangles_make_a_chain_and_the_round_guard_holds():
    n = 40
    e = (F(1) - np.arange(n, dtype=F)*F(0.5/n)).astype(F)
    t = np.zeros((n, 3, 3), F)
    t[:, 0] = -e[:, None]
    t[:, 1] = np.stack([e, -e, e], 1)
    t[:, 2] = np.stack([e, e, 0*e], 1)
    assert bh.build_ploc(t)[1] == n           # n - 1 levels of internal nodes + the leaf
    with pytest.raises(bh.NoProgress):
        bh.ploc_children(bh.morton_keys(t), t, max_rounds=n - 2)


def _meta(nodes, n, need, top):
    return dict(root=0 if n > 1 else bh.LEAF, numInternal=len(nodes), numTris=n, stackNeed=need, topCount=top, twoLeaves=0, inArena=0)


@pytest.mark.parametrize("n", [2, 3, 5, 64, 2049, 2100])
@pytest.mark.parametrize("build", [bh.build_lbvh, bh.build_ploc], ids=["lbvh", "ploc"])
def test_host_trees_pass_the_invariants(build, n):
    t = np.random.default_rng(n).uniform(-1, 1, (n, 3, 3)).astype(F)
    nodes, need, top = build(t)
    assert top == min(n - 1, bh.WALK_TOP_NODES)
    bh.check_tree(nodes, _meta(nodes, n, need, top), t, True, need + 1)
    # canonical form forgives internal ids: the same tree with its non-top ids permuted
    perm = np.arange(n - 1)
    rest = perm[top:].copy()
    np.random.default_rng(0).shuffle(rest)
    perm[top:] = rest
    moved = np.zeros_like(nodes)
    moved[perm] = nodes
    for f in ("left", "right"):
        v = moved[f]
        inner = (v & bh.LEAF) == 0
        v[inner] = perm[v[inner]]
    assert np.array_equal(bh.canonical(moved), bh.canonical(nodes))


def _broken(nodes, what):
    b = nodes.copy()
    if what == "tight_box":
        b["lmax"][3, 1] = np.nextafter(b["lmax"][3, 1], F(-np.inf))
    elif what == "duplicate_leaf":
        k = np.nonzero(b["left"] & bh.LEAF)[0][0]
        j = np.nonzero(b["right"] & bh.LEAF)[0][-1]
        b["left"][k] = b["right"][j]
    elif what == "swapped_bfs":
        for k in range(len(b)):
            for f in ("left", "right"):
                if b[f][k] in (1, 2):
                    b[f][k] = 3 - b[f][k]
        b[[1, 2]] = b[[2, 1]]
    elif what == "cycle":
        k = np.nonzero((b["left"] & bh.LEAF) == 0)[0][-1]
        b["left"][k] = 0
    return b


@pytest.mark.parametrize("what", ["tight_box", "duplicate_leaf", "swapped_bfs", "cycle", "stack_need", "no_stack"])
def test_invariant_checker_catches_broken_trees(what):
    n = 64
    t = np.random.default_rng(1).uniform(-1, 1, (n, 3, 3)).astype(F)
    nodes, need, top = bh.build_lbvh(t)
    meta = _meta(nodes, n, need, top)
    stack = need + 1
    if what == "stack_need":
        meta["stackNeed"] = need - 1
    elif what == "no_stack":
        stack = need
    else:
        nodes = _broken(nodes, what)
    with pytest.raises(AssertionError):
        bh.check_tree(nodes, meta, t, True, stack)

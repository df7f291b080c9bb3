"""The exact-tie corpus (tests/golden/ties.golden.npz, made by tests/golden/make_ties.py) against both CPU checkers.

The corpus holds what the reference's own Trace() (render.cpp:17-62) answered on rays almost all of which have two hits with the same t:
only its visit order names the winner.  Here, without a GPU: the reference compiled now answers the same bits (when oracle/_ref is
built), and the C restatement (oracle/tinsel_oracle.c) -- whose trace() walks its own copy of QueryBVH -- resolves every tie the same
way, primitive, t and every bit of the normal, and renders the same radiance and framebuffer.  tests/test_gpu_ties.py holds the HIP
kernels to the same records.

The corpus, counted from the reference alone by the generator (which asserts the floors: 1,000 exactly tied rays, 500 whose winner is not
the lowest-indexed of the tied primitives, 100 rays with a second hit within 1e-5 |t| that is not equal; `python tests/golden/make_ties.py`
prints the table again):
    dup_flat       prims  8  rays  7808  hit  6783  tied  6537  not lowest  4579  near   487  pairs with both winners 0
    dup_order      prims 12  rays  7808  hit  6982  tied  2912  not lowest  1497  near  1085  pairs with both winners 4
    dup_moving     prims 10  rays  7808  hit  6478  tied  6342  not lowest  5768  near   261  pairs with both winners 1
    dup_scene_bvh  prims 76  rays  7808  hit  7359  tied  5111  not lowest  2039  near   159  pairs with both winners 10
    dup_walked     prims  9  rays  7808  hit  6859  tied  5122  not lowest  2746  near   266  pairs with both winners 0
    dup_triangles  prims  3  rays  8048  hit  7255  tied     0  not lowest     0  near     0  pairs with both winners 0
                   inside the mesh: tied  2653  normals differ  2653  not lowest  2589 (+z pair 640, -z pair 1949)  contested 19 (tied and not contested 2649)
(dup_triangles ties inside one mesh, between a triangle and its repeat on vertices of its own: `tied` there counts the rays whose two
triangles give the same t, `normals differ` those where the two interpolated normals are not the same bits, `contested` the rays --
aimed at shared edges and vertices -- on which another of the mesh's triangles has a hit within 1e-5 |t|: they are compared bit for bit
like every other ray wherever the reference's own trees are walked; under a device-built mesh tree their t is held too, their normal not.)  A scan in index order
that kept the first of two equal hits would name the wrong primitive on every `not lowest` ray.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tinsel_amd import abi
from tests import oracle_api as oa
from tests.golden import make_ties as mt

needs_ref = pytest.mark.skipif(not oa.have_ref_trace(), reason="oracle/_ref not built, or built before ref_leaf_trace (`make -C oracle ref` where the reference is)")
FLT_MAX = np.float32(3.4028234663852886e38)


class Corpus:
    """ties.golden.npz, read once; rays are made again from their seed (and checked against the recorded CRC-32) on first use"""

    def __init__(self):
        with np.load(os.path.join(oa.GOLDEN, "ties.golden.npz")) as g:
            self.g = {k: g[k] for k in g.files}
        self._rows = {}

    def pack(self, name):
        return self.g[name + "_pack"].tobytes()

    def rows(self, name):
        if name not in self._rows:
            rows = mt.all_rays(name, self.g)
            rows.setflags(write=False)
            self._rows[name] = rows
        return self._rows[name]

    def records(self, name):
        """Trace()'s records: primitive (int32, -1: a miss), t, normal [n, 3]"""
        return self.g[name + "_prim"].astype(np.int32), self.g[name + "_t"], self.g[name + "_normal"]

    def tied_sets(self, name):
        """[n, P] bool: the primitives that attain the ray's minimum"""
        P = num_primitives(self.pack(name))
        return np.unpackbits(self.g[name + "_tied_sets"], axis=1, bitorder="little")[:, :P].astype(bool)

    def __getitem__(self, key):
        return self.g[key]


def num_primitives(blob):
    return int(abi.PackHeader.from_buffer_copy(blob[:C.sizeof(abi.PackHeader)]).num_primitives)


_corpus = None


def corpus():
    global _corpus
    if _corpus is None:
        _corpus = Corpus()
    return _corpus


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def check_records(name, got, want, what):
    (gp, gt, gn), (wp, wt, wn) = got, want
    assert np.array_equal(gp, wp), "%s %s: %d primitives differ" % (name, what, int((gp != wp).sum()))
    assert same_bits(gt, wt), "%s %s: %d t differ" % (name, what, int((gt.view(np.uint32) != wt.view(np.uint32)).sum()))
    assert same_bits(gn, wn), "%s %s: %d normals differ" % (name, what, int((gn.view(np.uint32) != wn.view(np.uint32)).any(axis=1).sum()))


@pytest.fixture(scope="module")
def port():
    if not oa.have_port():
        subprocess.run(["make", "-C", os.path.join(oa.ROOT, "oracle"), "port"], check=True)
    return oa.PortOracle()


def test_the_corpus_meets_its_floors():
    """from the recorded tables alone: the floors the generator asserted, and that an index-order scan would be caught on each scene"""
    c = corpus()
    assert c.g[mt.SCENES[0] + "_pack"].nbytes > 0
    assert os.path.getsize(os.path.join(oa.GOLDEN, "ties.golden.npz")) <= os.path.getsize(os.path.join(oa.GOLDEN, "fuzz.golden.npz"))
    for name in mt.SCENES:
        prim, t, nrm = c.records(name)
        sets = c.tied_sets(name)
        hit = prim >= 0
        assert len(c.rows(name)) == len(prim) and sets.shape[0] == len(prim)
        assert (t[~hit] == FLT_MAX).all() and not nrm[~hit].any() and not sets[~hit].any()
        assert sets[np.nonzero(hit)[0], prim[hit]].all()
        if name == "dup_triangles":
            pair = c[name + "_pair"]
            differ = (c[name + "_alt_normal"].view(np.uint32) != nrm.view(np.uint32)).any(axis=1) & pair
            assert pair.sum() >= mt.FLOOR_TIED and differ.sum() >= mt.FLOOR_NOT_LOWEST
            contested = c[name + "_contested"]
            assert contested.sum() <= 0.01*pair.sum() and (pair & ~contested).sum() >= mt.FLOOR_TIED
            continue
        tied = hit & (sets.sum(axis=1) > 1)
        not_lowest = tied & (prim != sets.argmax(axis=1))
        assert tied.sum() >= mt.FLOOR_TIED and not_lowest.sum() >= mt.FLOOR_NOT_LOWEST, name
        assert num_primitives(c.pack(name)) <= 80


@pytest.mark.parametrize("name", mt.SCENES)
def test_port_trace_resolves_every_tie_as_recorded(port, name):
    c = corpus()
    h = port.load_pack(c.pack(name))
    try:
        check_records(name, port.trace(h, c.rows(name)), c.records(name), "PortOracle.trace")
    finally:
        port.free(h)


@pytest.mark.parametrize("name", mt.SCENES)
def test_port_render_equals_the_recorded_passes(port, name):
    c = corpus()
    h = port.load_pack(c.pack(name))
    try:
        cam, opt = port.camera_options(h)
        accum, rad, _ = port.render_seeded(h, cam, opt, 0, mt.PASSES, want_accum=True, want_radiance=True, threads=4)
    finally:
        port.free(h)
    assert same_bits(rad, c[name + "_radiance"]), "%s: %d paths differ" % (
        name, int((rad.view(np.uint32) != c[name + "_radiance"].view(np.uint32)).any(axis=-1).sum()))
    assert same_bits(accum, c[name + "_accum"]), name


@needs_ref
@pytest.mark.parametrize("name", mt.SCENES)
def test_ref_trace_equals_the_recorded_and_the_minimum_over_primitive_intersect(name):
    c = corpus()
    R = oa.RefOracle()
    h = R.load_pack(c.pack(name))
    try:
        rows = c.rows(name)
        got = R.trace(h, rows)
        check_records(name, got, c.records(name), "RefOracle.trace")
        T = mt.tables(R, h, rows)
        s = mt.stats(T, got[0], got[1])            # (asserts: hit iff some primitive is hit, t the minimum's bits, the primitive attains it)
        assert np.array_equal(s["sets"].T, c.tied_sets(name))
        # the normal is FaceForward of the winning primitive's own
        for p in np.unique(got[0][got[0] >= 0]):
            sel = np.nonzero(got[0] == p)[0]
            _, _, n = R.primitive_intersect(h, int(p), rows[sel])
            assert same_bits(mt.face_forward(n, rows[sel, 3:6]), got[2][sel]), (name, p)
    finally:
        R.free(h)

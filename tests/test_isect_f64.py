"""tests/isect_f64.py (the float64 statement of the three leaf shapes the tolerance arm's tests lean on) against the reference's compiled
PrimitiveIntersect -- the only place the statement leans on the reference.  No GPU: host arithmetic on both sides.

Rays: the sets of tests/test_gpu_ray_query._rays (65,536 random, 4,096 axis-aligned, 4,096 starting on a surface).  Where two candidates
are close or t is near 0 the answer depends on rounding, so the comparison is on CLEAR rays: one primitive at the minimum, the second
candidate more than 1e-4 relative away, no hit within 1e-4 max(1, |o|) of the origin -- by the reference's table (_min_table) AND by the
statement's own (isect_f64.clear, which also sees the roots the reference does not report -- a sphere's near root behind the origin --
and leaves out a t that float32 cannot resolve to 1e-4: one just above the origin's threshold, a grazing hit).  On
those: the same primitive, and |t64 - t_ref| <= 1e-4 t64 -- the gap the definition of a clear ray already tolerates, so a condition, not a
measurement."""
import numpy as np
import pytest

import tinsel_amd
from tests import isect_f64 as f64
from tests import oracle_api as oa
from tests import test_gpu_ray_query as trq

pytestmark = pytest.mark.skipif(not oa.have_ref(), reason="oracle/_ref not built")

SCENES = ["cornell", "veach", "features", "motionblur"] + ["fuzz:%02d" % k for k in range(8)]


@pytest.mark.parametrize("name", SCENES)
def test_the_statement_is_the_references_primitive_intersect_on_clear_rays(name):
    R = oa.RefOracle()
    blob = trq._pack(name)
    h = R.load_pack(blob)
    try:
        rays = trq._rays(R, h, 20261016 + trq.SCENES.index(name))
        near = np.zeros(len(rays), bool)
        tmin, count, arg, second = trq._min_table(R, h, rays, near)
        S = f64.Statement(tinsel_amd.Scene(blob))
        assert S.num_primitives == R.num_primitives(h)
        # a mesh above MAX_BRUTE_TRIS triangles (motionblur's) has no float64 statement: the rays the reference sees it hit first are left out
        stated = np.isin(arg, S.brute_prims())
        assert stated.sum() >= 0.25*np.isfinite(tmin).sum(), name
        res = S.closest(rays, prims=S.brute_prims())
        hit = np.isfinite(tmin) & stated
        with np.errstate(invalid="ignore"):
            clear_ref = hit & (count == 1) & ((second - tmin) > 1e-4*tmin) & ~near
        clear = clear_ref & f64.clear(res)
        print("%-12s hit %6d  clear by the reference %6d  by both %6d" % (name, int(hit.sum()), int(clear_ref.sum()), int(clear.sum())))
        # (a ray that starts on a surface is not clear by construction: the share is of the others)
        elsewhere = np.arange(len(rays)) < trq.N_RANDOM + trq.N_AXIS
        assert (clear & elsewhere).sum() >= 0.85*(hit & elsewhere).sum(), name
        # a ray the reference misses and the statement calls clear is a lost hit on one side
        lost = ~np.isfinite(tmin) & f64.clear(res)
        assert not lost.any(), "%s: %d rays hit by the statement alone" % (name, int(lost.sum()))
        assert np.array_equal(res["primitive"][clear], arg[clear]), "%s: %d clear rays name another primitive" % (
            name, int((res["primitive"][clear] != arg[clear]).sum()))
        t64 = res["t"][clear]
        gap = np.abs(t64 - tmin[clear].astype(np.float64))/t64
        print("%-12s |t64 - t_ref|/t64: largest %.3e, median %.3e" % (name, gap.max(), np.median(gap)))
        assert (gap <= 1e-4).all(), name
        # the normal the reference reports for that primitive is the statement's shading normal, face-forwarded (float32 against float64)
        nref = trq._face_forward(trq._reference_normals(R, h, rays, np.where(clear, arg, -1)), rays[:, 4:7])
        ang = f64.angle(nref[clear], res["shading"][clear])
        # 1e-3 rad: another rule (a vertex order, a side, a pose) turns a normal by the angle between neighbouring vertex normals or by
        # pi, 1e-2 and more; float32's own error is that of the hit point over the shape's size, 3e-4 at the largest measured here
        print("%-12s angle to the reference's normal: largest %.3e rad" % (name, ang.max()))
        assert ang.max() <= 1e-3, name
    finally:
        R.free(h)


def test_the_shapes_at_hand_made_rays():
    """each shape once where the answer is known in closed form; the primitives of the features scene are found by type, not assumed"""
    S = f64.Statement(tinsel_amd.Scene(trq._pack("features")))
    abi = tinsel_amd.abi
    seen = set()
    for i, p in enumerate(S.prims):
        rays = np.zeros((1, 8), np.float32)
        rays[0, 7] = np.inf
        if p.type == abi.GEOM_SPHERE and not p.moving and "sphere" not in seen:
            c, r = p.start[0], p.radius*p.start[2]
            rays[0, 0:3], rays[0, 4:7] = c + np.array([0.0, 0.0, 3.0*r]), (0.0, 0.0, -1.0)
            out = S.intersect(i, rays)
            assert abs(out["t"][0] - 2.0*r) <= 1e-6*r and np.allclose(out["normal"][0], (0, 0, 1), atol=1e-6)
            rays[0, 0:3] = c                               # from inside: the far root, the normal turned towards the ray
            out = S.intersect(i, rays)
            assert abs(out["t"][0] - r) <= 1e-6*r and np.allclose(out["normal"][0], (0, 0, 1), atol=1e-6)
            seen.add("sphere")
        elif p.type == abi.GEOM_PLANE and "plane" not in seen:
            n, w = p.plane[:3], p.plane[3]
            assert abs(np.linalg.norm(n) - 1.0) <= 1e-6
            foot = -w*n + 0.25*np.cross(n, [0.3, 0.5, 0.7])            # a point of the plane
            rays[0, 0:3], rays[0, 4:7] = foot + 2.0*n, -n              # straight down from 2 above it
            out = S.intersect(i, rays)
            assert abs(out["t"][0] - 2.0) <= 1e-5 and np.allclose(out["normal"][0], n, atol=1e-6)
            rays[0, 4:7] = n                                            # away from it: no hit
            assert not np.isfinite(S.intersect(i, rays)["t"][0])
            seen.add("plane")
        elif p.type == abi.GEOM_MESH and not p.moving and p.tris is not None and "triangle" not in seen:
            pp, q, s = S.pose(i, np.zeros(1))
            tri = pp + f64.qrotate(np.repeat(q, 3, axis=0), s[0]*p.tris[0])      # triangle 0 in world space
            g = np.cross(tri[1] - tri[0], tri[2] - tri[0])
            g /= np.linalg.norm(g)
            centre = tri.mean(axis=0)
            for side in (1.0, -1.0):                                    # two-sided: from either side, the normal towards the ray
                rays[0, 0:3], rays[0, 4:7] = centre + side*0.5*g, -side*g
                one = S.intersect(i, rays)
                # (another triangle of the mesh may lie in between: then t is smaller, never larger)
                assert one["t"][0] <= 0.5 + 1e-5 and (one["t"][0] < 0.5 - 1e-5 or np.allclose(one["normal"][0], side*g, atol=1e-5))
            outside = tri[0] + 2.0*(tri[0] - centre)                    # past a corner: this triangle is not hit there
            rays[0, 0:3], rays[0, 4:7] = outside + 0.5*g, -g
            only = f64.Statement.__new__(f64.Statement)
            only.prims, only.boxes = [p], [None]
            keep = (p.tris, p.normals)
            p.tris, p.normals = p.tris[:1], None if p.normals is None else p.normals[:1]
            try:
                assert not np.isfinite(only.intersect(0, rays)["t"][0])
                rays[0, 0:3], rays[0, 4:7] = centre + 0.5*g, -g
                one = only.intersect(0, rays)
                assert abs(one["t"][0] - 0.5) <= 1e-5 and np.allclose(one["normal"][0], g, atol=1e-5)
            finally:
                p.tris, p.normals = keep
            seen.add("triangle")
    assert seen == {"sphere", "plane", "triangle"}, seen

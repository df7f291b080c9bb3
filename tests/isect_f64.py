"""A float64 statement of the three leaf shapes -- ray-sphere, ray-plane, ray-triangle -- and of a brute-force closest hit over a scene.

What the tolerance arithmetic arm (tinsel_fast.hip) is measured against: it cannot be held to the reference bit for bit, so it is held to
the OPERATION, stated here in plain numpy float64 with no tree walk, no early out and no float32 intermediate:
  * the pose of a primitive at the ray's time by the rule of prim_pose / InterpolateTransform (maths.h:1566): position and scale
    interpolated linearly, the quaternion interpolated linearly and then normalised;
  * ray-sphere as IntersectRaySphere states it (a = 1: the direction is taken as unit length): the smallest root > 0;
  * ray-plane as IntersectRayPlane: t = -(n.o + w)/(n.d), accepted when t > 0;
  * ray-triangle as IntersectRayTriTwoSided (ray_tri): two-sided, t >= 0, 0 <= v <= 1, w >= 0, v + w <= 1, in the mesh's own space;
  * a primitive is a candidate only for rays that reach its leaf box of the scene BVH (the reference's Trace() calls PrimitiveIntersect
    for exactly those: a rotating mesh leaves the box PrimitiveBounds joins from the two ends of the shutter), by the reference's slab test;
  * the closest hit is the smallest accepted t > 0 over the candidates.
Geometry comes from tinsel_amd.Scene (scene.desc): no oracle is needed.  tests/test_isect_f64.py pins this file to the reference's
PrimitiveIntersect; everything else that uses it leans on it alone.

Besides the hit, closest() says how far the answer is from depending on rounding -- the three conditions of a CLEAR ray plus two the
float64 roots make visible:
  count    primitives at the minimum                      second   the smallest t of the OTHER primitives
  near     some primitive has a root, of either sign, within 1e-4 max(1, |o|) of the origin
  edge     a candidate in front of (or within 1e-4 relative behind) the hit whose acceptance itself is marginal: a triangle met within
           1e-5 (barycentric) of its border, a sphere grazed (|discriminant| <= 1e-5 of its terms)
  boxed    a primitive would hit in front of (or within 1e-4 relative behind) the hit but the ray does not reach its leaf box
  cond     how many units of float32 roundoff, relative to t, the hit's t is uncertain by: the hit point's coordinates are sums of terms as
           large as |o|, the pose's position, the shape's extent and t, each rounded to half an ulp of its own size, and a displacement
           across the surface moves t by 1/cos(incidence) of itself: (|o| + |p| + extent + t)/(t cos).  A t just above the origin's
           threshold, or a grazing hit, is a t float32 does not resolve to 1e-4 whatever the arithmetic: not a clear ray either
"""
import ctypes as C

import numpy as np

from tinsel_amd import abi

NEAR = 1e-4            # |t| <= NEAR max(1, |o|): a candidate at the origin
CLEAR = 1e-4           # the two nearest candidates differ by more than CLEAR relative
COND = 1e-4/(8*2.0**-24)   # a clear ray's t is resolved to 1e-4 relative by eight roundings of the terms of `cond`
EDGE = 1e-5            # barycentric distance from a triangle's border / relative size of a sphere's discriminant below which acceptance is marginal
MAX_BRUTE_TRIS = 2000  # meshes above this get no float64 brute force
CHUNK = 1 << 21        # ray x triangle pairs per chunk (a dozen float64 temporaries of this many elements)


def _xform(t):
    return (np.array([t.p.x, t.p.y, t.p.z], np.float64), np.array([t.r.x, t.r.y, t.r.z, t.r.w], np.float64), np.float64(t.s))


def qrotate(q, v):
    """Rotate(q, v) = (q (v, 0) conj(q)).xyz for q [n, 4] (x, y, z, w; not assumed unit: the product scales by |q|^2 as the reference's does), v [n, 3]"""
    u, w = q[:, :3], q[:, 3:4]
    return (w*w - (u*u).sum(axis=1, keepdims=True))*v + 2.0*(u*v).sum(axis=1, keepdims=True)*u + 2.0*w*np.cross(u, v)


def face_forward(n, d):
    """FaceForward(n, -d): (-d . n) < 0 ? -n : n"""
    return np.where(((-d*n).sum(axis=1) < 0)[:, None], -n, n)


def _normalize(v):
    with np.errstate(all="ignore"):
        return v/np.sqrt((v*v).sum(axis=-1, keepdims=True))


class _Prim:
    pass


class Statement:
    """The primitives of a tinsel_amd.Scene in float64"""

    def __init__(self, scene):
        self.scene = scene                                     # (keeps the pack's memory alive)
        desc = scene.desc
        P = desc.num_primitives
        recs = (abi.Primitive*P).from_address(desc.primitives)
        self.prims = []
        for i in range(P):
            r, p = recs[i], _Prim()
            p.type = int(r.type)
            p.start, p.end = _xform(r.start_transform), _xform(r.end_transform)
            p.moving = bytes(r.start_transform) != bytes(r.end_transform)
            if p.type == abi.GEOM_SPHERE:
                p.radius = np.float64(r.geo.sphere.radius)
            elif p.type == abi.GEOM_PLANE:
                p.plane = np.array(list(r.geo.plane.plane), np.float64)
            else:
                g = r.geo.mesh
                nv, ni = int(g.num_vertices), int(g.num_indices)
                p.num_tris = ni//3
                p.tris = p.normals = None
                pos = np.ctypeslib.as_array((C.c_float*(nv*3)).from_address(g.positions)).reshape(nv, 3).astype(np.float64)
                c = 0.5*(pos.min(axis=0) + pos.max(axis=0))
                p.ball = (c, np.sqrt(((pos - c)**2).sum(axis=1).max()))     # (in mesh space)
                if p.num_tris <= MAX_BRUTE_TRIS:
                    idx = np.ctypeslib.as_array((C.c_uint32*ni).from_address(g.indices)).reshape(-1, 3).astype(np.int64)
                    p.tris = pos[idx]                          # [T, 3, 3]
                    if g.normals:
                        nr = np.ctypeslib.as_array((C.c_float*(nv*3)).from_address(g.normals)).reshape(nv, 3).astype(np.float64)
                        p.normals = nr[idx]
            self.prims.append(p)
        # The leaf boxes of the scene BVH, read as abi.BVHNode states the reference's node (bvh.h:9): a leaf (the top bit of the last word)
        # holds its primitive in left_index and PrimitiveBounds of it in lower / upper.  This is the pack's own data, written by the
        # reference's builder -- the one thing of the statement that is not restated; tests/test_isect_f64.py pins the result, and a ray whose
        # answer a box decides is not clear (`boxed`).
        assert C.sizeof(abi.BVHNode) == 32 and abi.BVHNode.left_index.offset == 24 and abi.BVHNode.right_index_leaf.offset == 28
        self.boxes = [None]*P
        n = desc.num_bvh_nodes
        if P > 1 and n > 0:
            f = np.ctypeslib.as_array((C.c_float*(n*8)).from_address(desc.bvh_nodes)).reshape(n, 8)
            u = f.view(np.uint32)
            for k in np.nonzero(u[:, 7] >> 31)[0]:
                assert self.boxes[int(u[k, 6])] is None, "a primitive with two leaves"
                self.boxes[int(u[k, 6])] = (f[k, 0:3].astype(np.float64), f[k, 3:6].astype(np.float64))
            assert all(b is not None for b in self.boxes), "a primitive without a leaf"

    @property
    def num_primitives(self):
        return len(self.prims)

    def brute(self, i):
        """can primitive i be stated here? (every sphere and plane; a mesh of at most MAX_BRUTE_TRIS triangles)"""
        p = self.prims[i]
        return p.type != abi.GEOM_MESH or p.tris is not None

    def brute_prims(self):
        return [i for i in range(len(self.prims)) if self.brute(i)]

    def all_brute(self):
        return all(self.brute(i) for i in range(len(self.prims)))

    def kind(self, i):
        return ("sphere", "plane", "mesh")[self.prims[i].type]

    def pose(self, i, time):
        """InterpolateTransform(start, end, time) -> (p [n, 3], q [n, 4], s [n])"""
        (p0, q0, s0), (p1, q1, s1) = self.prims[i].start, self.prims[i].end
        t = np.asarray(time, np.float64)[:, None]
        q = q0 + (q1 - q0)*t
        return p0 + (p1 - p0)*t, q/np.sqrt((q*q).sum(axis=1, keepdims=True)), (s0 + (s1 - s0)*t)[:, 0]

    def reached(self, i, rays):
        """IntersectRayAABBFast (intersection.h:373-397) on primitive i's leaf box, Min / Max as the reference's ternaries"""
        if self.boxes[i] is None:
            return np.ones(len(rays), bool)
        lo, hi = self.boxes[i]
        o, d = rays[:, 0:3].astype(np.float64), rays[:, 4:7].astype(np.float64)
        mn = lambda a, b: np.where(a < b, a, b)
        mx = lambda a, b: np.where(a > b, a, b)
        with np.errstate(all="ignore"):
            rcp = 1.0/d
            lmin = lmax = None
            for k in range(3):
                l1, l2 = (lo[k] - o[:, k])*rcp[:, k], (hi[k] - o[:, k])*rcp[:, k]
                lmin = mn(l1, l2) if k == 0 else mx(mn(l1, l2), lmin)
                lmax = mx(l1, l2) if k == 0 else mn(mx(l1, l2), lmax)
            return (lmax >= 0) & (lmax >= lmin)

    def intersect(self, i, rays, tmin=None):
        """Primitive i against rays [n, 8] (origin, time, direction, tmax) -> dict of
          t [n]       the accepted t > 0 -- > tmin [n] where given: the hit beyond a zone around the origin -- (inf: none)          normal [n, 3]   the unit geometric normal, face-forwarded against the ray
          shading [n, 3]  the normal PrimitiveIntersect returns (a mesh's interpolated vertex normals), face-forwarded
          near [n]    a root of either sign within NEAR max(1, |o|) of the origin
          edge_t [n]  the t of a marginal candidate (inf: none)"""
        p = self.prims[i]
        n = len(rays)
        o, d, time = rays[:, 0:3].astype(np.float64), rays[:, 4:7].astype(np.float64), rays[:, 3].astype(np.float64)
        thr = NEAR*np.maximum(1.0, np.abs(o).max(axis=1))
        tmin = np.zeros(n) if tmin is None else np.asarray(tmin, np.float64)
        out = dict(t=np.full(n, np.inf), normal=np.zeros((n, 3)), shading=np.zeros((n, 3)), near=np.zeros(n, bool), edge_t=np.full(n, np.inf),
                   scale=np.zeros(n))
        with np.errstate(all="ignore"):
            if p.type == abi.GEOM_PLANE:
                pl = p.plane
                den = (pl[:3]*d).sum(axis=1)
                t = -((pl[:3]*o).sum(axis=1) + pl[3])/den
                ok = (den != 0) & np.isfinite(t)
                out["near"] = ok & (np.abs(t) <= thr)
                hit = ok & (t > tmin)
                out["t"] = np.where(hit, t, np.inf)
                out["scale"][:] = abs(pl[3])/np.sqrt((pl[:3]**2).sum())
                nn = _normalize(np.broadcast_to(pl[:3], (n, 3)))
                out["normal"] = out["shading"] = np.where(hit[:, None], face_forward(nn, d), 0.0)
                return out
            pp, q, s = self.pose(i, time)
            if p.type == abi.GEOM_SPHERE:
                r = p.radius*s
                out["scale"] = np.sqrt((pp*pp).sum(axis=1)) + r
                qv = o - pp
                b = 2.0*(qv*d).sum(axis=1)
                qq = (qv*qv).sum(axis=1)
                c = qq - r*r
                disc = b*b - 4.0*c
                real = disc >= 0
                sq = np.sqrt(np.where(real, disc, 0.0))
                tt = -0.5*(b + np.where(b < 0, -1.0, 1.0)*sq)
                r0, r1 = tt, c/tt
                t0, t1 = np.minimum(r0, r1), np.maximum(r0, r1)
                t = np.where(t0 > tmin, t0, np.where(t1 > tmin, t1, np.inf))
                hit = real & np.isfinite(t)
                out["t"] = np.where(hit, t, np.inf)
                out["near"] = real & ((np.abs(t0) <= thr) | (np.abs(t1) <= thr))
                nn = _normalize(o + d*np.where(hit, t, 0.0)[:, None] - pp)
                out["normal"] = out["shading"] = np.where(hit[:, None], face_forward(nn, d), 0.0)
                graze = (np.abs(disc) <= EDGE*(b*b + 4.0*(qq + r*r))) & (-0.5*b > -thr)
                out["edge_t"] = np.where(graze, np.maximum(-0.5*b, 0.0), np.inf)
                return out
            # a mesh: the ray in mesh space (InverseTransformPoint / InverseTransformVector), every triangle
            assert p.tris is not None, "primitive %d: a mesh of %d triangles gets no float64 brute force" % (i, p.num_tris)
            qc = q*np.array([-1.0, -1.0, -1.0, 1.0])
            lo_, ld_ = qrotate(qc, o - pp)/s[:, None], qrotate(qc, d)/s[:, None]
            # rays whose line passes the mesh's bounding ball by more than its radius cannot hit
            c, rad = p.ball
            out["scale"] = np.sqrt((pp*pp).sum(axis=1)) + s*(np.sqrt((c*c).sum()) + rad)
            oc = c - lo_
            dist = np.sqrt((np.cross(oc, ld_)**2).sum(axis=1)/(ld_*ld_).sum(axis=1))
            cand = np.nonzero(~(dist > rad*(1.0 + 1e-6) + 1e-12))[0]
            T = len(p.tris)
            a_, ab, ac = p.tris[:, 0], p.tris[:, 1] - p.tris[:, 0], p.tris[:, 2] - p.tris[:, 0]
            nrm = np.cross(ab, ac)                                                      # [T, 3]
            step = max(1, CHUNK//max(1, T))
            for k0 in range(0, len(cand), step):
                sel = cand[k0:k0 + step]
                lo, ld = lo_[sel], ld_[sel]
                den = -(ld @ nrm.T)                                                     # [m, T]   d = dot(-dir, n)
                ap = lo[:, None, :] - a_[None, :, :]                                    # [m, T, 3]
                t = (ap*nrm[None]).sum(axis=2)/den
                e = np.cross(-ld[:, None, :], ap)
                v = (ac[None]*e).sum(axis=2)/den
                w = -(ab[None]*e).sum(axis=2)/den
                inside = (v >= 0) & (v <= 1) & (w >= 0) & (v + w <= 1)
                border = np.minimum(np.minimum(v, w), 1.0 - v - w)
                almost = (border >= -EDGE) & (v <= 1 + EDGE)
                th = thr[sel][:, None]
                out["near"][sel] = (almost & (np.abs(t) <= th)).any(axis=1)
                marginal = almost & (border <= EDGE) & (t > -th)
                out["edge_t"][sel] = np.where(marginal, np.maximum(t, 0.0), np.inf).min(axis=1)
                tt = np.where(inside & (t > tmin[sel][:, None]), t, np.inf)
                best = tt.argmin(axis=1)
                rows = np.arange(len(sel))
                tb = tt[rows, best]
                hit = np.isfinite(tb)
                out["t"][sel] = tb
                ng = nrm[best]*den[rows, best][:, None]                                 # n*sign: towards the ray, in mesh space
                sm = ng
                if p.normals is not None:
                    vb, wb = v[rows, best], w[rows, best]
                    nn3 = p.normals[best]
                    sm = (1.0 - vb - wb)[:, None]*nn3[:, 0] + vb[:, None]*nn3[:, 1] + wb[:, None]*nn3[:, 2]
                    sm = np.where(((sm*ng).sum(axis=1) < 0)[:, None], -sm, sm)
                qs, ss = q[sel], s[sel][:, None]
                gw = _normalize(qrotate(qs, ss*ng))
                sw = qrotate(qs, ss*sm)
                sw = np.where(((sw*sw).sum(axis=1) > 0)[:, None], _normalize(sw), gw)
                dd = d[sel]
                out["normal"][sel] = np.where(hit[:, None], face_forward(gw, dd), 0.0)
                out["shading"][sel] = np.where(hit[:, None], face_forward(sw, dd), 0.0)
            return out

    def closest(self, rays, restrict=True, prims=None, tmin=None):
        """The brute-force closest hit of rays [n, 8] over `prims` (default: every primitive) -> dict of t (inf: a miss), primitive (-1),
        normal, shading, count, second, near, edge, boxed (see the module's docstring).  tmin [n]: only hits with t > tmin count (the next
        surface of a ray that starts on one)"""
        n = len(rays)
        res = dict(t=np.full(n, np.inf), primitive=np.full(n, -1, np.int32), normal=np.zeros((n, 3)), shading=np.zeros((n, 3)),
                   count=np.zeros(n, np.int32), second=np.full(n, np.inf), near=np.zeros(n, bool), scale=np.zeros(n))
        edge_t, boxed_t = np.full(n, np.inf), np.full(n, np.inf)
        for i in (range(len(self.prims)) if prims is None else prims):
            r = self.intersect(i, rays, tmin)
            reach = self.reached(i, rays) if restrict else np.ones(n, bool)
            boxed_t = np.minimum(boxed_t, np.where(~reach, r["t"], np.inf))
            t = np.where(reach, r["t"], np.inf)
            res["near"] |= r["near"]
            edge_t = np.minimum(edge_t, r["edge_t"])
            less, equal = t < res["t"], (t == res["t"]) & np.isfinite(t)
            res["second"] = np.where(less, res["t"], np.minimum(res["second"], t))
            res["count"] = np.where(less, 1, res["count"] + equal)
            res["primitive"] = np.where(less, i, res["primitive"]).astype(np.int32)
            for k in ("normal", "shading"):
                res[k] = np.where(less[:, None], r[k], res[k])
            res["scale"] = np.where(less, r["scale"], res["scale"])
            res["t"] = np.where(less, t, res["t"])
        bound = np.where(np.isfinite(res["t"]), res["t"]*(1.0 + CLEAR), np.inf)
        res["edge"] = np.isfinite(edge_t) & (edge_t <= bound)
        o, d = rays[:, 0:3].astype(np.float64), rays[:, 4:7].astype(np.float64)
        with np.errstate(all="ignore"):
            cos = np.abs((res["normal"]*d).sum(axis=1))/np.sqrt((d*d).sum(axis=1))
            res["cond"] = np.where(np.isfinite(res["t"]), (np.sqrt((o*o).sum(axis=1)) + res["scale"] + res["t"])/(res["t"]*cos), np.inf)
        res["boxed"] = np.isfinite(boxed_t) & (boxed_t <= bound)
        return res


def clear(res):
    """The clear rays of a closest() result: one primitive at the minimum, the second candidate more than CLEAR relative away, no candidate
    at the origin -- and no candidate whose acceptance, or whose leaf box, rounding decides, and a t that float32 resolves to 1e-4"""
    with np.errstate(invalid="ignore"):
        return np.isfinite(res["t"]) & (res["count"] == 1) & ((res["second"] - res["t"]) > CLEAR*res["t"]) & ~res["near"] & ~res["edge"] & ~res["boxed"] & (res["cond"] <= COND)


def angle(a, b):
    """the angle between unit vectors [n, 3] in radians, accurate near 0 (atan2 of |a x b| and a . b)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.arctan2(np.sqrt((np.cross(a, b)**2).sum(axis=1)), (a*b).sum(axis=1))


def near_tie(S, rays, expected, primitive, t):
    """Rays that start on a surface and have a clear next surface `expected` [n], on which an arithmetic reports `primitive` [n] (-1: a
    miss) at `t` [n] instead: is that a near-tie at the origin, not a lost hit?  Two ways it can be:
      1. the reported primitive has a root within NEAR max(1, |o|) of the origin and is reported at such a t -- the start surface itself,
         or a neighbour that meets it there, on the positive side of a sign no arithmetic owns;
      2. the expected surface IS the start surface -- a sphere left through its inside, its near root within the origin's zone -- and the
         arithmetic's near root is exactly 0: IntersectRaySphere moves on to the far root only for `t0 < 0`, returns the 0, and Trace()'s
         `t > 0` drops the sphere altogether (the reference's own rule; the exact arm meets it on other rays).  The ray then goes on to the
         statement's closest hit over the OTHER primitives, and that -- or its miss -- is what must be reported.
    Anything else, the correct surface behind a lost one included, is a lost hit.  A mesh above MAX_BRUTE_TRIS triangles cannot be stated:
    a ray that reports one passes."""
    n = len(rays)
    o = rays[:, 0:3].astype(np.float64)
    thr = NEAR*np.maximum(1.0, np.abs(o).max(axis=1))
    primitive, t = np.asarray(primitive), np.asarray(t, np.float64)
    ok = np.zeros(n, bool)
    for p in np.unique(primitive):
        sel = np.nonzero(primitive == p)[0]
        if p >= 0 and not S.brute(int(p)):
            ok[sel] = True
        elif p >= 0:
            ok[sel] = S.intersect(int(p), rays[sel])["near"] & (t[sel] <= thr[sel])
    for b in np.unique(expected):
        if b < 0 or S.prims[int(b)].type != abi.GEOM_SPHERE:
            continue
        sel = np.nonzero((expected == b) & ~ok)[0]
        if not len(sel):
            continue
        left = S.intersect(int(b), rays[sel])["near"]
        rest = S.closest(rays[sel], prims=[i for i in S.brute_prims() if i != b], tmin=thr[sel])
        same = rest["primitive"] == primitive[sel]
        with np.errstate(invalid="ignore"):
            at = (primitive[sel] < 0) | (np.abs(rest["t"] - t[sel]) <= thr[sel] + CLEAR*rest["t"])
        ok[sel] = left & same & at
    return ok


PERCENTILES = (("median", 50.0), ("99th", 99.0), ("99.9th", 99.9), ("max", 100.0))


def error_margins(what, e_fast, e_exact, check=True, quiet=False):
    """The tolerance arm's error distribution against the exact arm's, both measured against float64 on the same rays: at the median, the
    99th and the 99.9th percentile the tolerance arm may be at most 4x the exact arm (every operation its build swaps in has at most twice
    the rounding error of the one it replaces: 2; a bound against an observed percentile: another 2), at the maximum 16x -- of the exact
    arm's own figure, so where that is 0 the tolerance arm's is 0 too.  Prints the figures, tolerance / exact and their ratio (TABLE lines:
    profiles/fast_arm_accuracy.md) and, with `check`, asserts the margins."""
    e_fast, e_exact = np.asarray(e_fast, np.float64), np.asarray(e_exact, np.float64)
    rows = [(label, np.percentile(e_exact, q), np.percentile(e_fast, q)) for label, q in PERCENTILES]
    ratio = lambda e, f: "%.2fx" % (f/e) if e > 0 else ("=" if f == 0 else "inf")
    if not quiet:
        print("TABLE %-44s n %6d  " % (what, len(e_fast)) + "  ".join("%s %.2e / %.2e (%s)" % (label, f, e, ratio(e, f)) for label, e, f in rows))
    if check:
        for label, e, f in rows:
            k = 16.0 if label == "max" else 4.0
            assert f <= k*e, "%s: at the %s the tolerance arm's error %.3e is %s the exact arm's %.3e (margin %gx)" % (what, label, f, ratio(e, f), e, k)
    return rows

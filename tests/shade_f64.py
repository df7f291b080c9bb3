"""A float64 statement of the shading leaves -- the Disney BSDF (eval, pdf, sample), the samplers under it, the camera ray and the light
sample -- the counterpart of tests/isect_f64.py for everything that is not an intersection.

What the tolerance arithmetic arm (tinsel_fast.hip) is measured against function by function (tests/test_gpu_fast_leaf.py): it cannot be
held to the reference bit for bit, so it is held to the OPERATION, stated here in plain numpy float64 with no float32 intermediate.  The
formulas are restated from the reference with line citations (disney.h, maths.h, util.h, intersection.h, probe.h), as tn_bsdf.h does;
tests/test_shade_f64.py pins this file to the reference's own functions.

  * The material is the RAW one of the pack (abi.Material): Cdlum / Ctint / Cspec0 (disney.h:306-310), the square root of the colour
    (:352), the clearcoat alpha and its logarithm (:387, :59-61) and the index of refraction (scene.h:72-78) are digested here in
    float64 -- the renderer's Mat128 is not read.
  * The random generator is integer arithmetic (maths.h:1036-1074) and restated as tests/accumulate_reference.raster_draws does; a
    Randf() is the draw converted to float32 and scaled by 2^-32, a value float64 holds exactly.
  * Inputs are the float32 rows the kernels get, taken as exact.

Every function is vectorised over rows [n, ...]; bsdf_sample also says which lobe it took and how many draws it used.  `near_flip_*`
say where the statement itself is within FLIP of a comparison going the other way: rows no arithmetic owns.
"""
import ctypes as C

import numpy as np

from tinsel_amd import abi
from tests import isect_f64 as f64

PI = np.pi
FLIP = 1e-6            # a comparison whose two sides differ by less than this is one rounding decides
# float literals of the reference that act as thresholds, at their float32 values: Max(0.001f, roughness) (disney.h:145), Max(1.e-6f, L.H) (:153),
# Lerp(.04f, 1.0f, FH) (:388)
ROUGHNESS_FLOOR, L_DOT_H_FLOOR, CLEARCOAT_F0 = float(np.float32(0.001)), float(np.float32(1.e-6)), float(np.float32(.04))

# the lobes BSDFSample can take, in the order disney.h meets them
LOBE_FRESNEL_GGX, LOBE_REFRACT, LOBE_TIR, LOBE_INSIDE, LOBE_COSINE, LOBE_GGX = range(6)
LOBE_NAMES = ("fresnel-ggx", "refract", "tir", "inside", "cosine", "ggx")
REFLECTED, TRANSMITTED, SPECULAR = 0, 1, 2      # BSDFType (disney.h:27-32)


def _dot(a, b):
    return (a*b).sum(axis=-1)


def _v3(v):
    return np.array([v.x, v.y, v.z], np.float64)


class Material64:
    """abi.Material digested in float64"""

    def __init__(self, m):
        self.raw = m
        self.color = _v3(m.color)
        for k in ("metallic", "subsurface", "specular", "roughness", "specular_tint", "clearcoat", "clearcoat_gloss", "transmission", "eta"):
            setattr(self, k, np.float64(getattr(m, k)))
        # disney.h:306-310
        c = self.color
        cdlum = .3*c[0] + .6*c[1] + .1*c[2]
        ctint = c/cdlum if cdlum > 0.0 else np.ones(3)
        self.cspec0 = f64_lerp(self.specular*.08*f64_lerp(np.ones(3), ctint, self.specular_tint), c, self.metallic)
        self.sqrt_color = np.sqrt(c)                                            # disney.h:352
        self.clearcoat_alpha = .1 + (.001 - .1)*self.clearcoat_gloss           # Lerp(.1, .001, clearcoatGloss), disney.h:387
        self.clearcoat_log_a2 = np.log(self.clearcoat_alpha**2)                 # GTR1's logf(a2), disney.h:59-61
        # GetIndexOfRefraction (scene.h:72-78)
        self.ior = 2.0/(1.0 - np.sqrt(0.08*self.specular)) - 1.0 if self.eta == 0.0 else self.eta

    def classes(self):
        """which of the classes of tests/test_gpu_fast_leaf.py this material is in"""
        t = self.transmission
        return {k for k, v in (("transmission=0", t == 0), ("0<transmission<1", 0 < t < 1), ("transmission=1", t == 1),
                               ("subsurface>0", self.subsurface > 0), ("clearcoat>0,alpha<1", self.clearcoat > 0 and self.clearcoat_alpha < 1),
                               ("metallic>0", self.metallic > 0), ("roughness<=0.001", self.roughness <= ROUGHNESS_FLOOR),
                               ("roughness>=0.5", self.roughness >= 0.5)) if v}


def f64_lerp(a, b, t):
    """Lerp (maths.h:77): a + (b - a)*t"""
    return a + (b - a)*t


def materials(scene):
    """[Material64] of a tinsel_amd.Scene's primitives, from the pack's raw records"""
    recs = (abi.Primitive*scene.desc.num_primitives).from_address(scene.desc.primitives)
    return [Material64(r.material) for r in recs]


# ---------------------------------------------------------------------------
# the pieces (disney.h:34-96)

def refract(wi, n, eta):
    """Refract (disney.h:34-47) -> (refracted [n] bool, wt [n, 3], sin2ThetaT [n])"""
    cos_i = _dot(n, wi)
    sin2_i = np.maximum(0.0, 1.0 - cos_i*cos_i)
    sin2_t = eta*eta*sin2_i
    ok = ~(sin2_t >= 1)
    cos_t = np.sqrt(np.where(ok, 1.0 - sin2_t, 0.0))
    wt = eta[:, None]*-wi + (eta*cos_i - cos_t)[:, None]*n
    return ok, np.where(ok[:, None], wt, 0.0), sin2_t


def schlick_fresnel(u):
    """SchlickFresnel (disney.h:49-54)"""
    m = np.clip(1.0 - u, 0.0, 1.0)
    return m**5


def gtr1(n_dot_h, a, log_a2=None):
    """GTR1 (disney.h:56-62)"""
    if a >= 1:
        return np.full(np.shape(n_dot_h), 1.0/PI)
    a2 = a*a
    t = 1.0 + (a2 - 1.0)*n_dot_h*n_dot_h
    return (a2 - 1.0)/(PI*(np.log(a2) if log_a2 is None else log_a2)*t)


def gtr2(n_dot_h, a):
    """GTR2 (disney.h:64-69)"""
    a2 = a*a
    t = 1.0 + (a2 - 1.0)*n_dot_h*n_dot_h
    return a2/(PI*t*t)


def smith_ggx(n_dot_v, alpha_g):
    """SmithGGX (disney.h:71-76)"""
    a, b = alpha_g*alpha_g, n_dot_v*n_dot_v
    return 1.0/(n_dot_v + np.sqrt(a + b - a*b))


def fr(v_dot_n, eta_i, eta_t):
    """Fr (disney.h:79-96) -> (F [n], SinThetaT2 [n])"""
    with np.errstate(all="ignore"):
        s2 = (eta_i/eta_t)**2*(1.0 - v_dot_n*v_dot_n)
        tir = s2 > 1.0
        l_dot_n = np.sqrt(np.where(tir, 0.0, 1.0 - s2))
        eta = eta_t/eta_i
        r1 = (v_dot_n - eta*l_dot_n)/(v_dot_n + eta*l_dot_n)
        r2 = (l_dot_n - eta*v_dot_n)/(l_dot_n + eta*v_dot_n)
        return np.where(tir, 1.0, 0.5*(r1*r1 + r2*r2)), s2


def safe_normalize(v):
    """SafeNormalize (maths.h:261-273), fallback 0"""
    m = _dot(v, v)
    with np.errstate(all="ignore"):
        return np.where((m > 0.0)[:, None], v/np.sqrt(m)[:, None], 0.0)


def basis_from_vector(w):
    """BasisFromVector (maths.h:1261-1275) -> u, v"""
    with np.errstate(all="ignore"):
        first = np.abs(w[:, 0]) > np.abs(w[:, 1])
        inv_a = 1.0/np.sqrt(w[:, 0]**2 + w[:, 2]**2)
        inv_b = 1.0/np.sqrt(w[:, 1]**2 + w[:, 2]**2)
        z = np.zeros(len(w))
        ua = np.stack([-w[:, 2]*inv_a, z, w[:, 0]*inv_a], axis=1)
        ub = np.stack([z, w[:, 2]*inv_b, -w[:, 1]*inv_b], axis=1)
        u = np.where(first[:, None], ua, ub)
    return u, np.cross(w, u)


# ---------------------------------------------------------------------------
# BSDFPdf, BSDFEval (disney.h:125-166, 296-405)

def _split(rows):
    r = np.asarray(rows, np.float64)
    return r[:, 0:3], r[:, 3:6], r[:, 6:9], r[:, 9], r[:, 10]


def bsdf_pdf(mat, eta_i, eta_o, n, V, L, terms=False):
    """BSDFPdf (disney.h:125-166).  terms: also the largest of the terms the two Lerps add and subtract, [n] -- where it dwarfs the
    result (a specular pdf far below the diffuse one at transmission 1) a float32 evaluation loses that many digits to cancellation"""
    with np.errstate(all="ignore"):
        below = _dot(L, n) <= 0.0
        pdf_below = f64_lerp(1.0/(2.0*PI)*mat.subsurface*0.5, 0.0, mat.transmission)                     # :136-139
        F, _ = fr(_dot(n, V), eta_i, eta_o)                                                               # :143
        a = max(ROUGHNESS_FLOOR, mat.roughness)
        half = safe_normalize(L + V)
        cos_h = np.abs(_dot(half, n))
        pdf_half = gtr2(cos_h, a)*cos_h
        pdf_spec = 0.25*pdf_half/np.maximum(L_DOT_H_FLOOR, _dot(L, half))                                         # :153
        pdf_diff = np.abs(_dot(L, n))*(1.0/PI)*(1.0 - mat.subsurface)                                     # :156
        above = f64_lerp(f64_lerp(pdf_diff, pdf_spec, 0.5), pdf_spec*F, mat.transmission)                 # :159-163
        pdf = np.where(below, pdf_below, above)
        if terms:
            return pdf, np.where(below, np.abs(pdf_below), np.maximum(np.maximum(pdf_diff, np.abs(pdf_spec)), np.abs(pdf_spec*F)))
        return pdf


def bsdf_eval(mat, eta_i, eta_o, N, V, L, terms=False):
    """BSDFEval (disney.h:296-405) -> f [n, 3].  terms: also the larger of |brdf| and |bsdf|, which the last Lerp adds and subtracts, [n, 3]"""
    with np.errstate(all="ignore"):
        n_dot_l, n_dot_v = _dot(N, L), _dot(N, V)
        H = L + V
        H = H/np.sqrt(_dot(H, H))[:, None]                                                                # Normalize: 0/0 where L == -V
        n_dot_h, l_dot_h = _dot(N, H), _dot(L, H)
        below = n_dot_l <= 0
        n = len(n_dot_l)
        a = max(ROUGHNESS_FLOOR, mat.roughness)
        Ds = gtr2(n_dot_h, a)
        Gs = smith_ggx(n_dot_v, a)*smith_ggx(n_dot_l, a)
        bsdf = np.zeros((n, 3))
        brdf = np.zeros((n, 3))
        if mat.transmission > 0.0:                                                                        # :316-341
            F, _ = fr(n_dot_v, eta_i, eta_o)
            through = mat.transmission*(1.0 - F)/np.abs(n_dot_l)*(1.0 - mat.metallic)
            FH, _ = fr(l_dot_h, eta_i, eta_o)
            Fs = f64_lerp(mat.cspec0[None, :], 1.0, FH[:, None])
            bsdf = np.where(below[:, None], through[:, None], (Gs*Ds)[:, None]*Fs)
        if mat.transmission < 1.0:                                                                        # :343-402
            inside = np.zeros((n, 3))
            if mat.subsurface > 0.0:
                FL, FV = schlick_fresnel(np.abs(n_dot_l)), schlick_fresnel(n_dot_v)
                Fd = (1.0 - 0.5*FL)*(1.0 - 0.5*FV)
                inside = (1.0/PI)*mat.sqrt_color[None, :]*mat.subsurface*Fd[:, None]*(1.0 - mat.metallic)
            FH = schlick_fresnel(l_dot_h)
            Fs = f64_lerp(mat.cspec0[None, :], 1.0, FH[:, None])
            FL, FV = schlick_fresnel(n_dot_l), schlick_fresnel(n_dot_v)
            Fd90 = 0.5 + 2.0*l_dot_h*l_dot_h*mat.roughness
            Fd = f64_lerp(1.0, Fd90, FL)*f64_lerp(1.0, Fd90, FV)
            Dr = gtr1(n_dot_h, mat.clearcoat_alpha, mat.clearcoat_log_a2)
            Fc = f64_lerp(CLEARCOAT_F0, 1.0, FH)
            Gr = smith_ggx(n_dot_l, .25)*smith_ggx(n_dot_v, .25)
            above = (1.0/PI)*Fd[:, None]*mat.color[None, :]*(1.0 - mat.metallic)*(1.0 - mat.subsurface) + (Gs*Ds)[:, None]*Fs + \
                (mat.clearcoat*Gr*Fc*Dr)[:, None]
            brdf = np.where(below[:, None], inside, above)
        f = f64_lerp(brdf, bsdf, mat.transmission)
        return (f, np.maximum(np.abs(brdf), np.abs(bsdf))) if terms else f


def near_flip_eval(mat, rows):
    """rows [n, 11] of BSDFEval / BSDFPdf on which the statement is within FLIP of a comparison going the other way: |n.L| (both
    functions branch on its sign), and -- where the material transmits -- SinThetaT2 - 1 of the Fr calls (disney.h:84)"""
    N, V, L, ei, eo = _split(rows)
    with np.errstate(all="ignore"):
        flip = np.abs(_dot(N, L)) < FLIP
        if mat.transmission > 0.0:
            H = safe_normalize(L + V)
            for c in (_dot(N, V), _dot(L, H)):
                flip |= np.abs(fr(c, ei, eo)[1] - 1.0) < FLIP
    return flip


# ---------------------------------------------------------------------------
# the generator (maths.h:1036-1074)

class Random:
    """Random(seed) for an array of seeds: the two-word state, Rand() and Randf()"""

    def __init__(self, seeds):
        with np.errstate(over="ignore"):
            self.s1 = np.uint32(315645664) + np.asarray(seeds, np.uint32)
            self.s2 = self.s1 ^ np.uint32(0x13ab45fe)

    def rand(self, where=None):
        """one Rand() on the rows `where` (default: all) -> the draw [n] (other rows: their state's word, not a draw)"""
        s1, s2 = self.s1, self.s2
        with np.errstate(over="ignore"):
            n1 = (s2 ^ ((s1 << np.uint32(5)) | (s1 >> np.uint32(27)))) ^ (s1*s2)
            n2 = n1 ^ ((s2 << np.uint32(12)) | (s2 >> np.uint32(20)))
        if where is None:
            self.s1, self.s2 = n1, n2
        else:
            self.s1, self.s2 = np.where(where, n1, s1), np.where(where, n2, s2)
        return self.s1

    def randf(self, where=None):
        """Randf() (maths.h:1063-1074): float(value)*(1.0f/float(0xffffffff)) -- the draw rounded to float32, times 2^-32 -- as float64"""
        return self.rand(where).astype(np.float32).astype(np.float64)*2.0**-32


# ---------------------------------------------------------------------------
# the samplers (maths.h:1278-1325, disney.h:184-204)

def uniform_sample_sphere(u1, u2):
    """UniformSampleSphere (maths.h:1278-1287)"""
    z = 1.0 - 2.0*u1
    r = np.sqrt(np.maximum(0.0, 1.0 - z*z))
    phi = 2.0*PI*u2
    return np.stack([r*np.cos(phi), r*np.sin(phi), z], axis=1)


def uniform_sample_hemisphere(z, u):
    """UniformSampleHemisphere (maths.h:1291-1302) from its two draws, in draw order"""
    w = np.sqrt(1.0 - z*z)
    phi = 2.0*PI*u
    return np.stack([np.cos(phi)*w, np.sin(phi)*w, z], axis=1)


def cosine_sample_hemisphere(u1, u2):
    """CosineSampleHemisphere over UniformSampleDisc (maths.h:1304-1310, 1319-1325)"""
    r, theta = np.sqrt(u1), 2.0*PI*u2
    sx, sy = r*np.cos(theta), r*np.sin(theta)
    return np.stack([sx, sy, np.sqrt(np.maximum(0.0, 1.0 - sx*sx - sy*sy))], axis=1)


def ggx_half_vector(a, r1, r2):
    """the GTR2 half vector in the local frame (disney.h:184-197): x, y, z = sin cos, sin sin, cos"""
    phi = r1*2.0*PI
    cos_t = np.sqrt((1.0 - r2)/(1.0 + (a*a - 1.0)*r2))
    sin_t = np.sqrt(np.maximum(0.0, 1.0 - cos_t*cos_t))
    return np.stack([sin_t*np.cos(phi), sin_t*np.sin(phi), cos_t], axis=1)


def bsdf_sample(mat, rows, seeds):
    """BSDFSample (disney.h:170-293) after BasisFromVector, rows [n, 8] = n(3) V(3) etaI etaO -> dict of
      L [n, 3], pdf [n], type [n], lobe [n] (LOBE_*), draws [n] (Randf() calls used), state [n, 2] (the generator's words afterwards),
      pdf_terms [n] (bsdf_pdf's `terms` at the sampled direction), dir_terms [n] (1, on a GGX lobe 1/sinThetaHalf: disney.h:188 takes
      sinThetaHalf = sqrt(1 - cosThetaHalf^2), and one rounding of that difference next to 1 turns the half vector by 2^-24/sinThetaHalf),
      near [n]: a comparison of the statement's own is within FLIP of going the other way (a draw against transmission / F / 0.5 /
      subsurface, sin2ThetaT against 1, SinThetaT2 against 1, half.view and the sampled n.L against 0)"""
    r = np.asarray(rows, np.float64)
    N, view, ei, eo = r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7]
    n = len(r)
    U, Vt = basis_from_vector(N)
    rng = Random(seeds)
    every = np.ones(n, bool)
    with np.errstate(all="ignore"):
        u_t = rng.randf()
        bsdf_branch = u_t < mat.transmission                                                              # :172
        F, s2 = fr(_dot(N, view), ei, eo)                                                                 # :175
        u_f = rng.randf(bsdf_branch)
        fresnel_ggx = bsdf_branch & (u_f < F)                                                             # :178
        refr = bsdf_branch & ~fresnel_ggx
        brdf_branch = ~bsdf_branch
        two = fresnel_ggx | brdf_branch
        r1 = rng.randf(two)                                                                               # Sample2D (:182, :241)
        r2 = rng.randf(two)
        u_half = rng.randf(brdf_branch)
        diffuse = brdf_branch & (u_half < 0.5)                                                            # :243
        u_ss = rng.randf(diffuse)
        inside = diffuse & (u_ss < mat.subsurface)                                                        # :246
        cosine = diffuse & ~inside
        z_in = rng.randf(inside)                                                                          # UniformSampleHemisphere's draws
        u_in = rng.randf(inside)
        ggx = fresnel_ggx | (brdf_branch & ~diffuse)

        ok, wt, sin2_t = refract(view, N, ei/eo)                                                          # :210-214
        lobe = np.select([fresnel_ggx, refr & ok, refr, inside, cosine], [LOBE_FRESNEL_GGX, LOBE_REFRACT, LOBE_TIR, LOBE_INSIDE, LOBE_COSINE], LOBE_GGX)
        draws = np.select([fresnel_ggx, refr, inside, cosine], [4, 2, 7, 5], 4)

        a = max(ROUGHNESS_FLOOR, mat.roughness)
        h = ggx_half_vector(a, r1, r2)
        half = U*h[:, 0:1] + Vt*h[:, 1:2] + N*h[:, 2:3]
        h_dot_v = _dot(half, view)
        half = np.where((h_dot_v <= 0.0)[:, None], -half, half)                                           # :200-201
        L_ggx = 2.0*_dot(view, half)[:, None]*half - view                                                 # :204
        d = cosine_sample_hemisphere(r1, r2)
        L_cos = U*d[:, 0:1] + Vt*d[:, 1:2] + N*d[:, 2:3]                                                  # :258
        d = uniform_sample_hemisphere(z_in, u_in)
        L_in = U*d[:, 0:1] + Vt*d[:, 1:2] - N*d[:, 2:3]                                                   # :251
        L = np.select([ggx[:, None], cosine[:, None], inside[:, None]], [L_ggx, L_cos, L_in], wt)
        lobe_pdf, lobe_terms = bsdf_pdf(mat, ei, eo, N, view, L, terms=True)
        pdf = np.where(refr, np.where(ok, (1.0 - F)*mat.transmission, 0.0), lobe_pdf)                    # :217, :223, :291
        pdf_terms = np.where(refr, np.abs(pdf), lobe_terms)
        dir_terms = np.where(ggx, 1.0/np.maximum(np.sqrt(h[:, 0]**2 + h[:, 1]**2), 2.0**-24), 1.0)
        btype = np.select([refr & ok, inside], [SPECULAR, TRANSMITTED], REFLECTED)

        near = np.abs(u_t - mat.transmission) < FLIP
        near |= bsdf_branch & ((np.abs(u_f - F) < FLIP) | (np.abs(s2 - 1.0) < FLIP))
        near |= refr & (np.abs(sin2_t - 1.0) < FLIP)
        near |= brdf_branch & (np.abs(u_half - 0.5) < FLIP)
        near |= diffuse & (np.abs(u_ss - mat.subsurface) < FLIP)
        near |= ggx & (np.abs(h_dot_v) < FLIP)
        near |= ~refr & (np.abs(_dot(L, N)) < FLIP)
    return dict(L=L, pdf=pdf, type=btype.astype(np.int32), lobe=lobe.astype(np.int32), draws=draws.astype(np.int32),
                state=np.stack([rng.s1, rng.s2], axis=1), near=near, pdf_terms=pdf_terms, dir_terms=dir_terms)


# ---------------------------------------------------------------------------
# CameraSampler::GenerateRay (util.h:45-79)

def generate_ray(camera, width, height, raster_xy):
    """the camera ray of raster points [n, 2] -> origin [n, 3], dir [n, 3].  rasterToWorld = cameraToWorld*screenToCamera*rasterToScreen
    (util.h:57-70) applied factor by factor in float64; the camera's rotation is taken as given (Mat33(Quat): columns q*e_k, maths.h:654-663)"""
    xy = np.asarray(raster_xy, np.float64)
    n = len(xy)
    f = np.tan(np.float64(camera.fov)*0.5)
    aspect = float(width)/float(height)
    sx, sy, sz = 2.0*xy[:, 0]/width - 1.0, 1.0 - 2.0*xy[:, 1]/height, np.ones(n)       # rasterToScreen of (x, y, 0, 1)
    cam = np.stack([f*aspect*sx, f*sy, -sz], axis=1)                                    # screenToCamera
    q = np.array([[camera.rotation.x, camera.rotation.y, camera.rotation.z, camera.rotation.w]], np.float64)
    rel = f64.qrotate(np.repeat(q, n, axis=0), cam)                                     # cameraToWorld's rotation; p - origin
    origin = np.repeat(_v3(camera.position)[None, :], n, axis=0)
    return origin, rel/np.sqrt(_dot(rel, rel))[:, None]


# ---------------------------------------------------------------------------
# PrimitiveSample (intersection.h:855-904)

def primitive_sample(S, i, times, seeds):
    """PrimitiveSample of primitive i of an isect_f64.Statement (a sphere or a mesh with vertex normals) -> dict of pos, normal [n, 3],
    state [n, 2]"""
    p = S.prims[i]
    rec = (abi.Primitive*S.scene.desc.num_primitives).from_address(S.scene.desc.primitives)[i]
    pp, q, s = S.pose(i, times)                                                         # InterpolateTransform (maths.h:1566)
    rng = Random(seeds)
    if p.type == abi.GEOM_SPHERE:
        u1 = rng.randf()
        u2 = rng.randf()
        local = uniform_sample_sphere(u1, u2)*p.radius                                  # :867
        pos = pp + f64.qrotate(q, s[:, None]*local)                                     # TransformPoint (maths.h:606-609)
        d = pos - pp
        nrm = d/np.sqrt(_dot(d, d))[:, None]
    else:
        assert p.type == abi.GEOM_MESH and p.tris is not None and p.normals is not None
        g = rec.geo.mesh
        T = int(g.num_indices)//3
        cdf = np.ctypeslib.as_array((C.c_float*T).from_address(g.cdf)).astype(np.float64)
        r = rng.randf()
        tri = np.minimum(np.searchsorted(cdf, r, side="left"), T - 1)                   # LowerBound, :880-881
        rt = np.sqrt(rng.randf())                                                       # UniformSampleTriangle (maths.h:1312-1317)
        u = 1.0 - rt
        v = rng.randf()*rt
        w = 1.0 - u - v
        a, b, c = p.tris[tri, 0], p.tris[tri, 1], p.tris[tri, 2]
        n1, n2, n3 = p.normals[tri, 0], p.normals[tri, 1], p.normals[tri, 2]
        pos = pp + f64.qrotate(q, s[:, None]*(u[:, None]*a + v[:, None]*b + w[:, None]*c))                  # :899
        nrm = safe_normalize(f64.qrotate(q, s[:, None]*(u[:, None]*n1 + v[:, None]*n2 + w[:, None]*n3)))    # :900
    return dict(pos=pos, normal=nrm, state=np.stack([rng.s1, rng.s2], axis=1))


# ---------------------------------------------------------------------------
# ProbeSample (probe.h:205-236)

def probe_sample(scene, seeds):
    """ProbeSample on the pack's probe -> dict of row, col [n], color [n, 3] (the texel, copied), dir [n, 3], pdf [n].  The binary searches
    compare float32 draws with float32 tables: exact in any arithmetic.  The tables themselves (pdfValuesX / Y, probe.h:31-79) are the
    pack's data; direction and solid-angle factor are float64"""
    d = scene.desc
    W, H = int(d.probe_width), int(d.probe_height)
    arr = lambda ptr, n: np.ctypeslib.as_array((C.c_float*n).from_address(ptr))
    cdf_y, pdf_y = arr(d.probe_cdf_y, H), arr(d.probe_pdf_y, H)
    cdf_x, pdf_x = arr(d.probe_cdf_x, W*H).reshape(H, W), arr(d.probe_pdf_x, W*H).reshape(H, W)
    data = arr(d.probe_data, W*H*4).reshape(H, W, 4)
    rng = Random(seeds)
    r1 = rng.randf().astype(np.float32)
    r2 = rng.randf().astype(np.float32)
    row = np.searchsorted(cdf_y, r1, side="left")                                       # LowerBound (probe.h:186-203), :214
    row_c = np.minimum(row, H - 1)
    col = np.array([np.searchsorted(cdf_x[j], x, side="left") for j, x in zip(row_c, r2)])     # :220
    col_c = np.minimum(col, W - 1)
    inside = (row < H) & (col < W)
    pdf = pdf_x[row_c, col_c].astype(np.float64)*pdf_y[row_c].astype(np.float64)        # :223
    u, v = col/float(W), row/float(H)                                                   # :225-226
    sin_t = np.sin(v*PI)
    with np.errstate(all="ignore"):
        pdf = np.where(sin_t == 0.0, 0.0, pdf*(W*H)/(2.0*PI*PI*sin_t))                  # :228-232
    theta, phi = v*PI, u*2.0*PI                                                         # ProbeUVToDir (probe.h:115-125)
    direction = np.stack([-np.sin(theta)*np.cos(phi), np.cos(theta), -np.sin(theta)*np.sin(phi)], axis=1)
    return dict(row=row, col=col, inside=inside, color=data[row_c, col_c, :3].copy(), dir=direction, pdf=pdf)


# ---------------------------------------------------------------------------
# errors as tests/test_gpu_fast_leaf.py measures them

def rel_error(x, x64):
    """|x - x64| relative to max(|x64|, 1e-6 max|row|), per element ([n] or [n, k]); 0 where both are 0"""
    x, x64 = np.asarray(x, np.float64), np.asarray(x64, np.float64)
    row = np.abs(x64).max(axis=-1, keepdims=True) if x64.ndim > 1 else np.abs(x64)
    den = np.maximum(np.abs(x64), 1e-6*row)
    with np.errstate(all="ignore"):
        e = np.abs(x - x64)/den
    return np.where((den == 0) & (x == x64), 0.0, e)

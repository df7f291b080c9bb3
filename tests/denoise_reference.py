"""The feature-guided denoise stage (tinsel_hip_denoise*, include/tinsel_hip.h) stated in numpy float32 with the host libm's expf -- the
reference of tests/test_gpu_denoise.py, pinned itself to the reference's NonLocalMeansFilter by tests/test_denoise_abi.py.  Every
operation below is one float32 operation, in the order the statement gives (no fused multiply-add anywhere); a pixel meets its taps with
fx ascending outside and fy ascending inside, which is what walking the offsets (ox outer, oy inner) and skipping the taps outside the
frame does for every pixel at once."""
import ctypes as C
import ctypes.util

import numpy as np

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.expf.restype = C.c_float
_libm.expf.argtypes = [C.c_float]
F = np.float32
ALBEDO, NORMAL, DEPTH = 1, 2, 4


def expf(a):
    """libm expf, element by element, as float32"""
    a = np.asarray(a, F)
    f = _libm.expf
    return np.array([f(v) for v in a.ravel().tolist()], F).reshape(a.shape)


class Params:
    """tinsel_hip_denoise_params by name (anything with these attributes will do, the ctypes mirror included)"""

    def __init__(self, radius, patch_radius, k_color, k_albedo=0.0, k_normal=0.0, k_depth=0.0, demodulate=0, albedo_floor=0.01):
        self.radius, self.patch_radius = int(radius), int(patch_radius)
        self.k_color, self.k_albedo, self.k_normal, self.k_depth = F(k_color), F(k_albedo), F(k_normal), F(k_depth)
        self.demodulate, self.albedo_floor = int(demodulate), F(albedo_floor)


def _ratio(num, den):
    """num/den in float32, 0 where den == 0"""
    ok = den != 0
    with np.errstate(all="ignore"):
        return np.where(ok, num/np.where(ok, den, F(1.0)), F(0.0)).astype(F)


def _taps(H, W, radius):
    """(ox, oy, destination slices, source slices) of the window's offsets in the filter's order, clipped to the frame"""
    for ox in range(-radius, radius + 1):
        for oy in range(-radius, radius + 1):
            x0, x1 = max(0, -ox), min(W, W - ox)
            y0, y1 = max(0, -oy), min(H, H - oy)
            if x0 < x1 and y0 < y1:
                yield (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


def _length_sq(d):
    """dx*dx + dy*dy + ..., left to right"""
    s = d[..., 0]*d[..., 0]
    for k in range(1, d.shape[-1]):
        s = s + d[..., k]*d[..., k]
    return s


def average_filter(image, radius):
    """AverageFilter (nlm.cpp:4-33): the clipped box, summed fx outer and fy inner, times 1.0f/count"""
    H, W = image.shape[:2]
    total = np.zeros_like(image, F)
    count = np.zeros((H, W), np.int32)
    for dst, src in _taps(H, W, radius):
        total[dst] = total[dst] + image[src]
        count[dst] += 1
    rc = F(1.0)/count.astype(F)
    return (total*rc[..., None]).astype(F)


def prepare(beauty, planes, features, p):
    """-> (U [H, W, 4], d [H, W, 3], a [H, W, 3], n [H, W, 3], z [H, W])"""
    beauty = np.asarray(beauty, F)
    H, W = beauty.shape[:2]
    by_bit, k = {}, 0
    for bit in (ALBEDO, NORMAL, DEPTH):
        if features & bit:
            by_bit[bit] = np.asarray(planes[k], F)
            k += 1
    c = _ratio(beauty[..., :3], beauty[..., 3:4])
    zero3 = np.zeros((H, W, 3), F)
    a = _ratio(by_bit[ALBEDO][..., :3], by_bit[ALBEDO][..., 3:4]) if features & ALBEDO else zero3
    n = _ratio(by_bit[NORMAL][..., :3], by_bit[NORMAL][..., 3:4]) if features & NORMAL else zero3
    z = _ratio(by_bit[DEPTH][..., 0], by_bit[DEPTH][..., 2]) if features & DEPTH else np.zeros((H, W), F)
    if p.demodulate:
        assert features & ALBEDO
        d = np.where(a < F(p.albedo_floor), F(p.albedo_floor), a).astype(F)
        u = (c/d).astype(F)
    else:
        d = np.ones((H, W, 3), F)
        u = c
    U = np.zeros((H, W, 4), F)
    U[..., :3] = u
    return U, d, a, n, z


def denoise_reference(beauty, planes=None, features=0, params=None):
    """beauty [H, W, 4], planes [popcount(features), H, W, 4] in ascending bit order -> the denoised image [H, W, 4] (w = 1)"""
    p = params
    features = int(features)
    assert 0 <= features <= 7
    U, d, a, n, z = prepare(beauty, planes, features, p)
    H, W = U.shape[:2]
    M = average_filter(U, int(p.patch_radius))
    kc, ka, kn, kd = F(p.k_color), F(p.k_albedo), F(p.k_normal), F(p.k_depth)
    total = np.zeros((H, W), F)
    acc = np.zeros((H, W, 3), F)
    with np.errstate(all="ignore"):
        for dst, src in _taps(H, W, int(p.radius)):
            e = kc*_length_sq(M[dst] - M[src])
            if features & ALBEDO:
                e = e + ka*_length_sq(a[dst] - a[src])
            if features & NORMAL:
                e = e + kn*_length_sq(n[dst] - n[src])
            if features & DEPTH:
                den = z[dst]*z[dst] + z[src]*z[src]
                dz = z[dst] - z[src]
                ok = den != 0
                e = e + kd*np.where(ok, dz*dz/np.where(ok, den, F(1.0)), F(0.0)).astype(F)
            weight = expf(-e)
            acc[dst] = acc[dst] + U[src][..., :3]*weight[..., None]
            total[dst] = total[dst] + weight
        rc = F(1.0)/total
        out = np.ones((H, W, 4), F)
        out[..., :3] = (acc*rc[..., None])*d
    assert out.dtype == F
    return out

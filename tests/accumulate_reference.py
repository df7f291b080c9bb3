"""CpuRenderer::AddSample (the reference's render.cpp:401-445, as oracle/tinsel_oracle.c restates it) over whole passes of caller-chosen radiance,
in numpy float32 with the host libm's expf -- the reference of tests/test_gpu_accumulate_support.py, and the filter arithmetic
tests/test_accumulate_support.py checks.  A pixel receives the samples of one pass in the raster order of the pixels that generated them, pass
after pass; every operation below is one float32 operation, in the order the C code performs it (no fused multiply-add anywhere)."""
import ctypes as C
import ctypes.util

import numpy as np

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.expf.restype = C.c_float
_libm.expf.argtypes = [C.c_float]
F = np.float32


def expf(a):
    """libm expf, element by element, as float32"""
    a = np.asarray(a, F)
    f = _libm.expf
    return np.array([f(v) for v in a.ravel().tolist()], F).reshape(a.shape)


def constructor_offset(width, falloff):
    """Filter::Filter (render.h): offset = expf(-falloff*width*width)"""
    return expf(-F(falloff)*F(width)*F(width))[()]


def gaussian(x, falloff, offset):
    """Filter::Gaussian (render.h:29-32): max(0, expf(-falloff*x*x) - offset)"""
    x = np.asarray(x, F)
    return np.maximum(F(0), expf(-F(falloff)*x*x) - F(offset))


def raster_draws(W, H, seed):
    """The first two Randf() of Random(i + j*W + seed) (maths.h:1036-1091) for every pixel: x[H, W], y[H, W]"""
    i, j = np.meshgrid(np.arange(W, dtype=np.uint32), np.arange(H, dtype=np.uint32))
    with np.errstate(over="ignore"):
        s1 = np.uint32(315645664) + (i + j*np.uint32(W) + np.uint32(seed))
        s2 = s1 ^ np.uint32(0x13ab45fe)
        out = []
        for _ in range(2):
            s1 = (s2 ^ ((s1 << np.uint32(5)) | (s1 >> np.uint32(27)))) ^ (s1*s2)
            s2 = s1 ^ ((s2 << np.uint32(12)) | (s2 >> np.uint32(20)))
            out.append(s1.astype(F)*F(1.0/4294967296.0))
    return out[0], out[1]


def clamp_length(v, max_length):
    """ClampLength (maths.h:1577-1589) of v[..., 3]"""
    with np.errstate(all="ignore"):
        l = np.sqrt(v[..., 0]*v[..., 0] + v[..., 1]*v[..., 1] + v[..., 2]*v[..., 2])
        scaled = v*(F(max_length)/l)[..., None]
    return np.where((l > F(max_length))[..., None], scaled, v).astype(F)


def add_passes(accum, radiance, seeds, filt, clamp):
    """accum[H, W, 4] + the passes radiance[passes, H, W, 4] (rgbx), filt = (type, width, falloff, offset): a new array"""
    ftype, fw, falloff, offset = int(filt[0]), F(filt[1]), F(filt[2]), F(filt[3])
    acc = np.array(accum, F)
    H, W = acc.shape[:2]
    lo, hi = 2 + int(np.floor(fw)), 1 + int(np.ceil(fw))          # (one more than the footprint reaches: r + fw may round up to the next integer)
    K = lo + hi + 1
    px, py = np.meshgrid(np.arange(W, dtype=np.int32), np.arange(H, dtype=np.int32))
    for s in range(radiance.shape[0]):
        x, y = raster_draws(W, H, seeds[s])
        rx, ry = x + px.astype(F), y + py.astype(F)
        c = clamp_length(np.asarray(radiance[s, :, :, :3], F), clamp)
        startX, startY = np.maximum(0, np.trunc(rx - fw).astype(np.int32)), np.maximum(0, np.trunc(ry - fw).astype(np.int32))
        endX, endY = np.minimum(np.trunc(rx + fw).astype(np.int32), W - 1), np.minimum(np.trunc(ry + fw).astype(np.int32), H - 1)
        if ftype != 0:
            # the weights of every footprint column / row of every sample, evaluated once
            wx, wy = np.zeros((K, H, W), F), np.zeros((K, H, W), F)
            for k in range(K):
                mx, my = startX + k <= endX, startY + k <= endY
                wx[k][mx] = gaussian((startX + k).astype(F)[mx] - rx[mx], falloff, offset)
                wy[k][my] = gaussian((startY + k).astype(F)[my] - ry[my], falloff, offset)
        for oj in range(-lo, hi + 1):
            for oi in range(-lo, hi + 1):
                # pixels P and the sample generated at P + (oi, oj), where that is inside the frame
                x0, x1, y0, y1 = max(0, -oi), min(W, W - oi), max(0, -oj), min(H, H - oj)
                if x0 >= x1 or y0 >= y1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                G = (slice(y0 + oj, y1 + oj), slice(x0 + oi, x1 + oi))
                kx, ky = px[P] - startX[G], py[P] - startY[G]
                cover = (kx >= 0) & (px[P] <= endX[G]) & (ky >= 0) & (py[P] <= endY[G])
                if not cover.any():
                    continue
                with np.errstate(all="ignore"):
                    if ftype == 0:
                        add = np.concatenate([c[G], np.ones(cover.shape + (1,), F)], axis=-1)
                    else:
                        w = (np.take_along_axis(wx[(slice(None),) + G], np.clip(kx, 0, K - 1)[None], 0)[0] *
                             np.take_along_axis(wy[(slice(None),) + G], np.clip(ky, 0, K - 1)[None], 0)[0])
                        add = np.concatenate([c[G]*w[..., None], w[..., None]], axis=-1)
                    acc[P] = np.where(cover[..., None], acc[P] + add, acc[P])
    return acc

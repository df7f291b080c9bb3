"""The yardstick of the sample-map tests: tinsel_hip_render_sample_map adds, per pixel q, the samples of levels 0 .. counts[q] - 1 -- level t
the path a render starts for q in pass pass_begin + t -- by AddSample, a sample that does not exist skipped.  That is
accumulate_reference.add_passes with ONE extra term, cover &= live[t][generating pixel], fed the oracle's own per-sample radiance
(render_seeded(..., want_radiance=True)) and its pass seeds (pass_seed); the oracle is the one the view-batch tests use.  add_passes itself
is imported, not edited, and stays the statement of the unmasked case.  Radiance is computed once per (pack, camera, options, pass_begin,
levels), shared and left unchanged."""
import functools
import os

import numpy as np

from tinsel_amd import abi
from tests import accumulate_reference as ar
from tests import views_reference as vr

F = np.float32
W, H = vr.W, vr.H       # 40 x 24: three by two accumulate tiles, both edges ragged

oracle = vr.oracle
pack_bytes = vr.pack_bytes
frame = vr.frame


def add_levels(accum, radiance, seeds, filt, clamp, live):
    """accum[H, W, 4] + the levels radiance[levels, H, W, 3+] of the pixels live[levels, H, W] says have one, filt = (type, width, falloff,
    offset): a new array.  add_passes line for line, with `& live[s][G]` in the cover."""
    ftype, fw, falloff, offset = int(filt[0]), F(filt[1]), F(filt[2]), F(filt[3])
    acc = np.array(accum, F)
    Hh, Ww = acc.shape[:2]
    lo, hi = 2 + int(np.floor(fw)), 1 + int(np.ceil(fw))          # (one more than the footprint reaches: r + fw may round up to the next integer)
    K = lo + hi + 1
    px, py = np.meshgrid(np.arange(Ww, dtype=np.int32), np.arange(Hh, dtype=np.int32))
    for s in range(radiance.shape[0]):
        if not live[s].any():
            continue
        x, y = ar.raster_draws(Ww, Hh, seeds[s])
        rx, ry = x + px.astype(F), y + py.astype(F)
        c = ar.clamp_length(np.asarray(radiance[s, :, :, :3], F), clamp)
        startX, startY = np.maximum(0, np.trunc(rx - fw).astype(np.int32)), np.maximum(0, np.trunc(ry - fw).astype(np.int32))
        endX, endY = np.minimum(np.trunc(rx + fw).astype(np.int32), Ww - 1), np.minimum(np.trunc(ry + fw).astype(np.int32), Hh - 1)
        if ftype != 0:
            wx, wy = np.zeros((K, Hh, Ww), F), np.zeros((K, Hh, Ww), F)
            for k in range(K):
                mx, my = startX + k <= endX, startY + k <= endY
                wx[k][mx] = ar.gaussian((startX + k).astype(F)[mx] - rx[mx], falloff, offset)
                wy[k][my] = ar.gaussian((startY + k).astype(F)[my] - ry[my], falloff, offset)
        for oj in range(-lo, hi + 1):
            for oi in range(-lo, hi + 1):
                x0, x1, y0, y1 = max(0, -oi), min(Ww, Ww - oi), max(0, -oj), min(Hh, Hh - oj)
                if x0 >= x1 or y0 >= y1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                G = (slice(y0 + oj, y1 + oj), slice(x0 + oi, x1 + oi))
                kx, ky = px[P] - startX[G], py[P] - startY[G]
                cover = (kx >= 0) & (px[P] <= endX[G]) & (ky >= 0) & (py[P] <= endY[G])
                cover &= live[s][G]                                 # the one extra term: the generating pixel has a sample at this level
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


def live_levels(counts):
    """live[t][j][i] = counts[j][i] > t for t below the largest count"""
    counts = np.asarray(counts)
    return np.arange(int(counts.max()) if counts.size else 0)[:, None, None] < counts[None]


@functools.lru_cache(maxsize=None)
def _radiance(name, cam_bytes, opt_bytes, pass_begin, levels):
    cam, opt = abi.Camera.from_buffer_copy(cam_bytes), abi.Options.from_buffer_copy(opt_bytes)
    O = oracle()
    h = O.load_pack(pack_bytes(name))
    try:
        accum, rad, _ = O.render_seeded(h, cam, opt, pass_begin, levels, threads=min(16, os.cpu_count() or 1), want_radiance=True)
        seeds = tuple(int(O.pass_seed(pass_begin + t)) & 0xffffffff for t in range(levels))
    finally:
        O.free(h)
    accum.setflags(write=False)
    rad.setflags(write=False)
    return accum, rad, seeds


def oracle_levels(name, cam, opt, pass_begin, levels):
    """(the oracle's accumulator of the passes [pass_begin, pass_begin + levels) from zero, its radiance [levels, H, W, 3], their seeds)"""
    return _radiance(name, bytes(cam), bytes(opt), int(pass_begin), int(levels))


def filter_of(opt):
    return (opt.filter.type, opt.filter.width, opt.filter.falloff, opt.filter.offset)


def statement(name, cam, opt, pass_begin, counts, start=None):
    """what a sample-map call with `counts` [H, W] at pass_begin leaves in out: float32 [H, W, 4], from zero or on top of `start`"""
    counts = np.asarray(counts)
    acc = np.zeros(counts.shape + (4,), F) if start is None else np.array(start, F)
    if opt.max_depth < 1 or not counts.any():
        return acc
    _, rad, seeds = oracle_levels(name, cam, opt, pass_begin, int(counts.max()))
    return add_levels(acc, rad, seeds, filter_of(opt), opt.clamp, live_levels(counts))


def random_counts(seed, top=5, width=W, height=H):
    """a seeded map in 0 .. top, zeros and tops included"""
    return np.random.default_rng(seed).integers(0, top + 1, (height, width)).astype(np.uint16)


def plan(slot_limit, width, height, counts):
    """tinsel_hip_plan_sample_map in a few lines: (levels per batch, batches, total paths, largest count), None where it refuses"""
    npix, top = width*height, 0xfffffffe
    if npix > top:
        return None
    counts = np.asarray(counts, np.int64)
    levels = max(1, min(int(slot_limit), top)//npix)
    most = int(counts.max())
    return levels, -(-most//levels), int(counts.sum()), most


def batch_offsets(counts, t0, levels):
    """the exclusive prefix sum of a batch [t0, t0 + levels): W*H + 1 entries, the last one its path count"""
    share = np.clip(np.asarray(counts, np.int64).ravel() - t0, 0, levels)
    return np.concatenate([[0], np.cumsum(share)])

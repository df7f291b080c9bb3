"""The rule of tinsel_hip_render_id_mattes (include/tinsel_hip.h) as sequential numpy float32 -- the statement tests/test_gpu_id_mattes.py
holds the kernels to, and tests/test_id_mattes_abi.py checks against tests/accumulate_reference.add_passes.

Structured like add_passes: the same raster_draws, footprints and gaussian; a pixel visits the samples of one pass in the raster order of
the pixels that generated them, pass after pass.  A candidate whose footprint covers the pixel with weight w > 0: total += w; a slot that
holds its id: weight += w; else the first empty slot takes (id, w); else residual += w.  Every add is one float32 add.  At the end the
slots are ranked: weight descending, ties by ascending id, empty slots last."""
import numpy as np

from tests.accumulate_reference import gaussian, raster_draws

F = np.float32
ID_MISS, ID_EMPTY = -1, -2


def rank(ids, weights):
    """ids / weights [K, H, W] sorted per pixel: weight descending, ties by ascending id, empty slots last"""
    order = np.lexsort((ids, -weights.astype(np.float64), ids == ID_EMPTY), axis=0)
    return np.take_along_axis(ids, order, 0), np.take_along_axis(weights, order, 0)


def id_mattes(path_ids, seeds, filt, slots, owned=None, ranked=True):
    """path_ids[passes, H, W] int (ID_MISS where the path left the scene), filt = (type, width, falloff, offset), owned[H, W] bool: the
    pixels whose samples this rank generates (None: all).  Returns {"ids": int32 [slots, H, W], "weights": float32 [slots, H, W],
    "residual": [H, W], "total": [H, W]}; ranked = False leaves the slots in first-seen order."""
    ftype, fw, falloff, offset = int(filt[0]), F(filt[1]), F(filt[2]), F(filt[3])
    path_ids = np.asarray(path_ids, np.int32)
    H, W = path_ids.shape[1:]
    owned = np.ones((H, W), bool) if owned is None else np.asarray(owned, bool)
    ids = np.full((slots, H, W), ID_EMPTY, np.int32)
    weights = np.zeros((slots, H, W), F)
    residual, total = np.zeros((H, W), F), np.zeros((H, W), F)
    lo, hi = 2 + int(np.floor(fw)), 1 + int(np.ceil(fw))          # (one more than the footprint reaches: r + fw may round up to the next integer)
    K = lo + hi + 1
    px, py = np.meshgrid(np.arange(W, dtype=np.int32), np.arange(H, dtype=np.int32))
    for s in range(path_ids.shape[0]):
        x, y = raster_draws(W, H, seeds[s])
        rx, ry = x + px.astype(F), y + py.astype(F)
        startX, startY = np.maximum(0, np.trunc(rx - fw).astype(np.int32)), np.maximum(0, np.trunc(ry - fw).astype(np.int32))
        endX, endY = np.minimum(np.trunc(rx + fw).astype(np.int32), W - 1), np.minimum(np.trunc(ry + fw).astype(np.int32), H - 1)
        if ftype != 0:
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
                SP = (slice(None),) + P
                kx, ky = px[P] - startX[G], py[P] - startY[G]
                cover = (kx >= 0) & (px[P] <= endX[G]) & (ky >= 0) & (py[P] <= endY[G]) & owned[G]
                if not cover.any():
                    continue
                if ftype == 0:
                    w = np.ones(cover.shape, F)
                else:
                    w = (np.take_along_axis(wx[(slice(None),) + G], np.clip(kx, 0, K - 1)[None], 0)[0] *
                         np.take_along_axis(wy[(slice(None),) + G], np.clip(ky, 0, K - 1)[None], 0)[0])
                counts = cover & (w > 0)
                c = path_ids[s][G]
                total[P] = np.where(counts, total[P] + w, total[P])
                held = (ids[SP] == c[None]) & counts[None]
                weights[SP] = np.where(held, weights[SP] + w[None], weights[SP])
                new = counts & ~held.any(axis=0)
                empty = ids[SP] == ID_EMPTY
                claim = empty & (np.cumsum(empty, axis=0) == 1) & new[None]         # the first empty slot
                ids[SP] = np.where(claim, c[None], ids[SP])
                weights[SP] = np.where(claim, w[None], weights[SP])
                over = new & ~claim.any(axis=0)
                residual[P] = np.where(over, residual[P] + w, residual[P])
    if ranked:
        ids, weights = rank(ids, weights)
    return {"ids": ids, "weights": weights, "residual": residual, "total": total}

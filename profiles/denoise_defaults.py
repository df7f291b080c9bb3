"""Chooses tinsel_hip_denoise_params' defaults on the CPU (no GPU needed): the host statement of the denoise stage
(tests/denoise_reference.py) on the reference's own renders (oracle/_ref) of cornell and features_probe at 64 x 64 and 4 spp, scored by
the mean squared error of the denoised linear radiance against the reference's render of the same frame at 1024 spp.  The guide planes
are built from the reference alone: the camera records of tests/test_gpu_radiance_query._starts, the reference's Trace() on them
(RefOracle.trace), the pack's colours, accumulated by tests/accumulate_reference.add_passes with the scene's own filter.

    python profiles/denoise_defaults.py            # prints the tables of profiles/denoise_defaults.md

Also checks the two conditions tests/test_gpu_denoise.py asks of cornell: a lower error than the noisy frame, and the wall edge where
the 1024-spp render has it."""
import ctypes as C
import itertools
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import oracle_api as oa                                     # noqa: E402
from tests.accumulate_reference import add_passes                      # noqa: E402
from tests.denoise_reference import Params, denoise_reference          # noqa: E402
from tests.test_gpu_radiance_query import _starts                      # noqa: E402
from tinsel_amd import abi                                             # noqa: E402

W = H = 64
SPP, REF_SPP = 4, 1024
SCENES = ("cornell", "features_probe")


def colour(img):
    w = img[..., 3:4]
    return np.where(w != 0, img[..., :3]/np.where(w != 0, w, 1), 0).astype(np.float32)


def case(R, name):
    """(noisy accumulator, planes [3, H, W, 4], 1024-spp colour)"""
    h = R.load_pack(os.path.join(oa.GOLDEN, name + ".pack"))
    cam, opt = R.camera_options(h)
    opt = opt.copy()
    opt.width, opt.height = W, H
    noisy, _, _ = R.render_seeded(h, cam, opt, 0, SPP)
    clean, _, _ = R.render_seeded(h, cam, opt, 0, REF_SPP)
    starts = _starts(R, cam, W, H, SPP)
    rows = np.stack([starts[f] for f in ("ox", "oy", "oz", "dx", "dy", "dz", "time")], axis=1).astype(np.float32)
    prim, t, nrm = R.trace(h, rows)
    hit = prim >= 0
    cols = np.array([[c.x, c.y, c.z] for c in (R.primitive(h, k).material.color for k in range(R.num_primitives(h)))], np.float32)
    feat = {n: np.zeros((len(rows), 4), np.float32) for n in abi.FEATURE_NAMES}
    feat["albedo"][hit, :3] = cols[prim[hit]]
    feat["normal"][hit, :3] = nrm[hit]
    th = t[hit]
    feat["depth"][hit, 0], feat["depth"][hit, 1], feat["depth"][hit, 2] = th, th*th, np.float32(1.0)
    seeds = [int(R.pass_seed(s)) for s in range(SPP)]
    filt = (opt.filter.type, opt.filter.width, opt.filter.falloff, opt.filter.offset)
    planes = np.stack([add_passes(np.zeros((H, W, 4), np.float32), feat[n].reshape(SPP, H, W, 4), seeds, filt, np.inf) for n in abi.FEATURE_NAMES])
    R.free(h)
    return noisy, planes, colour(clean)


CASES = None


def score(kw):
    """the mean squared error of one setting on every scene (a pool worker: the cases are the parent's)"""
    p = Params(**kw)
    return [mse(denoise_reference(CASES[n][0], CASES[n][1], 7, p)[..., :3], CASES[n][2]) for n in SCENES]


def mse(a, b):
    return float(np.mean((a.astype(np.float64) - b.astype(np.float64))**2))


def edge(planes, row):
    """column of the largest horizontal albedo step along `row`"""
    a = colour(planes[0])[row]
    return int(np.argmax(np.abs(np.diff(a, axis=0)).sum(axis=1)))


def steepest(image, row, lo, hi):
    g = np.abs(np.diff(image[row, :, :3].astype(np.float64), axis=0)).sum(axis=1)
    return lo + int(np.argmax(g[lo:hi]))


def main():
    R = oa.RefOracle()
    cases = {n: case(R, n) for n in SCENES}
    for n, (noisy, planes, clean) in cases.items():
        print("%s: noisy %d spp against %d spp: mse %.6f" % (n, SPP, REF_SPP, mse(colour(noisy), clean)))

    global CASES
    CASES = cases
    noise = [mse(colour(cases[n][0]), cases[n][2]) for n in SCENES]
    # the score of a setting: the mean over the scenes of its error relative to the noisy frame's, so that each scene counts alike
    rel = lambda s: sum(v/n0 for v, n0 in zip(s, noise))/len(noise)
    pool = multiprocessing.get_context("fork").Pool(min(16, os.cpu_count() or 1))

    def scores(settings):
        return list(zip(settings, pool.map(score, settings)))

    def table(title, rows):
        print("\n" + title)
        print("| " + " | ".join(list(rows[0][0]) + list(SCENES) + ["relative"]) + " |")
        print("|" + "---|"*(len(rows[0][0]) + len(SCENES) + 1))
        for kw, s in sorted(rows, key=lambda r: rel(r[1])):
            print("| " + " | ".join(["%g" % v for v in kw.values()] + ["%.6f" % v for v in s] + ["%.4f" % rel(s)]) + " |")

    base = dict(radius=4, patch_radius=1, k_color=4.0, k_albedo=64.0, k_normal=4.0, k_depth=64.0, demodulate=0, albedo_floor=0.01)
    grid = []
    for kc, ka, kn, kd, dm in itertools.product((0.25, 0.5, 1.0, 2.0, 4.0, 16.0), (0.0, 4.0, 16.0, 64.0), (0.0, 1.0, 4.0, 16.0), (0.0, 4.0, 16.0, 64.0), (0, 1)):
        if dm and ka == 0.0:
            continue                            # (demodulated colours of two albedos are not comparable: only with the albedo term)
        grid.append(dict(base, k_color=kc, k_albedo=ka, k_normal=kn, k_depth=kd, demodulate=dm))
    rows = sorted(scores(grid), key=lambda r: rel(r[1]))
    short = lambda kw: {k: kw[k] for k in ("k_color", "k_albedo", "k_normal", "k_depth", "demodulate")}
    table("coefficients at radius 4, patch radius 1 (the 20 best, the 4 worst of %d)" % len(rows), [(short(k), s) for k, s in rows[:20] + rows[-4:]])
    for name, pick in (("no guide term", lambda k: k["k_albedo"] == k["k_normal"] == k["k_depth"] == 0.0),
                       ("the albedo term", lambda k: k["k_albedo"] > 0 and not k["demodulate"]),
                       ("demodulation", lambda k: k["demodulate"])):
        kw, s = next((k, s) for k, s in rows if pick(k))
        print("best with %s: %s -> %s, relative %.4f" % (name, short(kw), ["%.6f" % v for v in s], rel(s)))
    best = rows[0][0]
    print("best:", best)
    rows = sorted(scores([dict(best, radius=r, patch_radius=pr) for r in (2, 3, 4, 6, 8) for pr in (0, 1, 2)]), key=lambda r: rel(r[1]))
    table("radii at the best coefficients", [({k: kw[k] for k in ("radius", "patch_radius")}, s) for kw, s in rows])
    best = rows[0][0]
    # factors of two around the best coefficients, at the best radii
    near = lambda v: (0.0, 1.0, 4.0) if v == 0.0 else (v/2, v, v*2)
    rows = sorted(scores([dict(best, k_color=kc, k_albedo=ka, k_normal=kn, k_depth=kd) for kc, ka, kn, kd in itertools.product(
        near(best["k_color"]), near(best["k_albedo"]), near(best["k_normal"]), near(best["k_depth"]))]), key=lambda r: rel(r[1]))
    table("refinement at radius %d, patch radius %d (the 16 best of %d)" % (best["radius"], best["patch_radius"], len(rows)),
          [(short(k), s) for k, s in rows[:16]])
    # the defaults: the best row -- or, within half a percent of it, the best row that uses every plane (the two scenes have no two
    # surfaces of one albedo and one normal at two depths; a scene that has should not meet a depth term of zero)
    floor = rel(rows[0][1])*1.005
    best = next(k for k, s in rows if rel(s) <= floor and k["k_albedo"] > 0 and k["k_normal"] > 0 and k["k_depth"] > 0) if any(
        rel(s) <= floor and k["k_albedo"] > 0 and k["k_normal"] > 0 and k["k_depth"] > 0 for k, s in rows) else rows[0][0]
    rows = sorted(scores([dict(best, k_albedo=max(best["k_albedo"], 16.0), demodulate=1, albedo_floor=f) for f in (0.001, 0.01, 0.05, 0.1, 0.2, 0.5)]),
                  key=lambda r: rel(r[1]))
    table("albedo floor (with demodulation and k_albedo at least 16, the rest as the best)", [({"albedo_floor": kw["albedo_floor"]}, s) for kw, s in rows])
    best = dict(best, albedo_floor=rows[0][0]["albedo_floor"])
    print("\ndefaults: " + " ".join("%s=%g" % (k, best[k]) for k in ("radius", "patch_radius", "k_color", "k_albedo", "k_normal", "k_depth", "demodulate",
                                                                      "albedo_floor")))

    # the conditions of tests/test_gpu_denoise.py's last test, on the reference's renders, with the library's defaults where it is built
    try:
        import tinsel_amd
        d = tinsel_amd.denoise_params()
        chosen = Params(**d.as_dict())
        print("\nthe library's defaults:", d.as_dict())
    except Exception as e:                      # pragma: no cover
        print("\n(library not built: %s) checking the best row instead" % e)
        chosen = Params(**best)
    noisy, planes, clean = cases["cornell"]
    out = denoise_reference(noisy, planes, 7, chosen)
    print("cornell: mse noisy %.6f -> denoised %.6f" % (mse(colour(noisy), clean), mse(out[..., :3], clean)))
    for row in (H//2, H//3, 2*H//3):
        x = edge(planes, row)
        lo, hi = max(0, x - 4), min(W - 1, x + 5)
        print("row %d: albedo edge at column %d; steepest step within 4 columns of it: 1024 spp %d, denoised %d, noisy %d" % (
            row, x, steepest(clean, row, lo, hi), steepest(out, row, lo, hi), steepest(colour(noisy), row, lo, hi)))


if __name__ == "__main__":
    main()

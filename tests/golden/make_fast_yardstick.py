"""Writes tests/golden/fast_yardstick.json: how far the reference's own two builds -- IEEE (oracle/_ref/libtinsel_ref.so) and as its makefile
builds it, -O3 -ffast-math (libtinsel_ref_fast.so) -- are off each other's track, per scene and depth, on the camera paths
tests/test_gpu_fast_accuracy.py asks the two GPU arms for: the scene's own camera, a 50 x 37 frame, 3 passes, max_depth 1, 2 and the pack's
own.  A path is off track when max|d rgb| > 1e-3 max(1e-3, max|rgb|) of the IEEE build's value (tests/test_gpu_fast.py's rule).  Host only:
    python -m tests.golden.make_fast_yardstick
The file holds recorded results only; the GPU test allows the tolerance arm 4x these shares plus 0.5 % of the paths."""
import json
import os

import numpy as np

from tests import oracle_api as oa
from tests.test_gpu_ray_query import _pack

SCENES = ["cornell", "veach", "features", "glass", "motionblur", "many_spheres", "cornell_probe", "ajax_standin_96"]
W, H, PASSES = 50, 37, 3


def main():
    builds = [oa.RefOracle(), oa.RefOracle(fast=True)]
    shares = {}
    for name in SCENES:
        blob = _pack(name)
        rad = {}
        for k, R in enumerate(builds):
            h = R.load_pack(blob)
            cam, opt = R.camera_options(h)
            own = opt.max_depth
            opt.width, opt.height = W, H
            for label, depth in (("1", 1), ("2", 2), ("own", own)):
                opt.max_depth = depth
                rad[k, label] = R.render_seeded(h, cam, opt, 0, PASSES, want_accum=False, want_radiance=True)[1].reshape(-1, 3)
            R.free(h)
        shares[name] = {}
        for label in ("1", "2", "own"):
            e, f = rad[0, label], rad[1, label]
            off = np.abs(f - e).max(axis=-1) > 1e-3*np.maximum(1e-3, np.abs(e).max(axis=-1))
            shares[name][label] = round(float(off.mean()), 6)
        print("%-16s %s" % (name, shares[name]))
    out = {"width": W, "height": H, "passes": PASSES, "off_track_share": shares}
    with open(os.path.join(oa.GOLDEN, "fast_yardstick.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()

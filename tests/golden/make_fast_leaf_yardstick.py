"""Writes tests/golden/fast_leaf_yardstick.json: on how many rows the reference's own two builds -- IEEE (oracle/_ref/libtinsel_ref.so) and as
its makefile builds it, -O3 -ffast-math (libtinsel_ref_fast.so) -- make ProbeSample pick DIFFERENT texels of features_probe from the same
seeds: the rows of tests/test_gpu_fast_leaf.py's probe table (65,536 seeds: fast_leaf_rows.probe_seeds).  Host only:
    python -m tests.golden.make_fast_leaf_yardstick
The file holds recorded results only; the GPU test lets the tolerance arm's texel differ from the exact arm's on 4x this share plus 0.5 %
of the rows."""
import json
import os

import numpy as np

from tests import fast_leaf_rows as flr
from tests import oracle_api as oa
from tests.test_gpu_ray_query import _pack

SCENE = "features_probe"


def main():
    seeds = flr.probe_seeds()
    colour = []
    for R in (oa.RefOracle(), oa.RefOracle(fast=True)):
        h = R.load_pack(_pack(SCENE))
        colour.append(R.probe(h, seeds)[1])
        R.free(h)
    differ = (colour[0] != colour[1]).any(axis=1)
    out = {"scene": SCENE, "rows": int(len(seeds)), "texel_differs_share": round(float(differ.mean()), 6)}
    print(out)
    with open(os.path.join(oa.GOLDEN, "fast_leaf_yardstick.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()

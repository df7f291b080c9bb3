"""Times the reduction of an SH gather query against the query's tracing kernels (run from the repository root, on an MI355X):

    python profiles/gather_sh_measure.py probe|texel [REPEATS]          # default 7 repeats

probe: cornell, 256 points x 4096 samples, sphere mode, order 2 -- the shape of a light-probe bake.
texel: ajax_standin_96, the first-hit points of its camera tiled to 2^18 points x 16 samples, cosine mode, order 2 -- a light map.
Device entries on a torch tensor, depth 4, exact arithmetic, kernel timing on (tinsel_hip_kernel_times: one record per call).  Per
repeat, interleaved: gather_sh, then gather on the same points.  Reported, as medians with min .. max over the repeats, in ms:
k_gather_sh_reduce, the sum of every other kernel of the SH query without and with k_generate_gather ("tracing"), and k_gather_reduce of
the plain gather -- the yardstick whose code does not change.  A library without the SH entry (another build loaded through
TINSEL_HIP_LIB for an A/B) reports the plain gather alone.  Prints one JSON line."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tinsel_amd                       # noqa: E402
from tinsel_amd import abi              # noqa: E402

SHAPES = {"probe": ("cornell", 256, 4096, "sphere"), "texel": ("ajax_standin_96", 1 << 18, 16, "cosine")}
DEPTH, ORDER, WARM = 4, 2, 2


def main(argv):
    shape = argv[1] if len(argv) > 1 else "probe"
    repeats = int(argv[2]) if len(argv) > 2 else 7
    name, n, samples, mode = SHAPES[shape]
    scene = tinsel_amd.Scene.load_pack(os.path.join("tests", "golden", name + ".pack"))
    r = tinsel_amd.create_gpu_renderer(scene)
    cam = abi.Camera.from_buffer_copy(scene.camera)
    points, _, primitive, normal = r.first_hit_points(cam, 64, 64)
    hit = primitive >= 0
    # (probe: spread over the frame's hits, not its first rows)
    pick = (np.arange(n)*(int(hit.sum())//n if n < hit.sum() else 1)) % int(hit.sum())
    pts = tinsel_amd.gather_points(points[hit][pick], normal[hit][pick], samples)
    dev_pts = torch.from_numpy(pts.view(np.float32).reshape(n, 8).copy()).cuda()
    have_sh = hasattr(r._L, "tinsel_hip_gather_sh_device")

    def sh():
        out = r.gather_sh(dev_pts, samples, DEPTH, ORDER, mode)
        torch.cuda.synchronize()
        return out

    def plain():
        out = r.gather(dev_pts, samples, DEPTH, mode)
        torch.cuda.synchronize()
        return out

    for _ in range(WARM):
        if have_sh:
            sh()
        plain()
    r.enable_kernel_timing(True)
    rows = {"k_gather_sh_reduce": [], "tracing": [], "tracing_and_generate": [], "k_gather_reduce": [], "plain_tracing": []}
    for _ in range(repeats):
        if have_sh:
            coef = sh()
            t = {k: v[1] for k, v in r.kernel_times().items()}
            rows["k_gather_sh_reduce"].append(t.pop("k_gather_sh_reduce"))
            rows["tracing_and_generate"].append(sum(t.values()))
            rows["tracing"].append(sum(v for k, v in t.items() if k != "k_generate_gather"))
        mean = plain()
        t = {k: v[1] for k, v in r.kernel_times().items()}
        rows["k_gather_reduce"].append(t.pop("k_gather_reduce"))
        rows["plain_tracing"].append(sum(v for k, v in t.items() if k != "k_generate_gather"))
    check = None
    if have_sh:         # band 0 is Y0 times the mean, to rounding: the two queries traced the same paths
        a, b = coef[:, 0, :3].double(), mean[:, :3].double()*float(np.float32(0.28209479))
        check = float(((a - b).abs()/(b.abs() + 1e-30)).max())
    r.close()
    stat = lambda t: {"median": round(float(np.median(t)), 4), "min": round(min(t), 4), "max": round(max(t), 4)} if t else None
    print(json.dumps({"shape": shape, "scene": name, "points": n, "samples": samples, "mode": mode, "order": ORDER, "max_depth": DEPTH,
                      "repeats": repeats, "library": os.environ.get("TINSEL_HIP_LIB", "in-tree"), "ms": {k: stat(v) for k, v in rows.items()},
                      "band0_vs_mean_largest_relative_difference": check}))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

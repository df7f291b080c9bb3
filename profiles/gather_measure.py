"""Times a gather query's device entry against the same paths as a radiance query (run from the repository root, on an MI355X):

    python profiles/gather_measure.py [SCENE [LOG2_POINTS [SAMPLES [MAX_DEPTH]]]]        # default: cornell 16 64 4

The points are the first-hit points of the scene's camera at a square frame of 2^LOG2_POINTS pixels (misses dropped, the hits tiled up to
the count, seed_k = k*SAMPLES).  A: tinsel_hip_gather_radiance_device, cosine mode, no starts_out.  B: tinsel_hip_trace_radiance_device on a
device tensor holding A's own starts_out (written once, before the timed window): the same paths, 48 bytes a path in and 16 out.
End to end: 3 warm-up rounds, then REPEATS rounds of A, B, A, B ... on torch's current stream, each call between a synchronise and a
synchronise on the host clock; medians, and the spread as min .. max.  Kernel times: two more calls of each with kernel timing on
(tinsel_hip_kernel_times), outside the timed window.  Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tinsel_amd                       # noqa: E402
from tinsel_amd import abi              # noqa: E402

WARM, REPEATS = 3, 15


def main(argv):
    name = argv[1] if len(argv) > 1 else "cornell"
    log2n, samples, depth = (int(argv[k]) if len(argv) > k else d for k, d in ((2, 16), (3, 64), (4, 4)))
    n = 1 << log2n
    scene = tinsel_amd.Scene.load_pack(os.path.join("tests", "golden", name + ".pack"))
    r = tinsel_amd.create_gpu_renderer(scene)
    cam = abi.Camera.from_buffer_copy(scene.camera)
    side = 1 << ((log2n + 1)//2)
    points, _, primitive, normal = r.first_hit_points(cam, side, side)
    hit = primitive >= 0
    pick = np.arange(n) % int(hit.sum())
    pts = tinsel_amd.gather_points(points[hit][pick], normal[hit][pick], samples)
    dev_pts = torch.from_numpy(pts.view(np.float32).reshape(n, 8).copy()).cuda()
    mean, starts = r.gather(dev_pts, samples, depth, "cosine", return_starts=True)
    torch.cuda.synchronize()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0)*1000.0

    a = lambda: r.gather(dev_pts, samples, depth, "cosine")
    b = lambda: r.radiance(starts, depth)
    for _ in range(WARM):
        a(), b()
    ta, tb = [], []
    for _ in range(REPEATS):
        ta.append(timed(a))
        tb.append(timed(b))
    # the same paths: B's results, reduced here, are A's means to a few ulp (torch's sum is not sequential in s)
    rad = r.radiance(starts, depth).view(n, samples, 4)[..., :3].sum(dim=1)/samples
    worst = float(((rad - mean[:, :3]).abs()/(mean[:, :3].abs() + 1e-6)).max())

    r.enable_kernel_timing(True)
    kernels = {}
    for label, fn in (("gather", a), ("radiance", b)):
        per = []
        for _ in range(2):
            fn()
            per.append({k: round(v[1], 4) for k, v in r.kernel_times().items()})
        kernels[label] = per
    r.close()
    stat = lambda t: {"median": round(float(np.median(t)), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
    print(json.dumps({"scene": name, "points": n, "samples": samples, "max_depth": depth, "repeats": REPEATS,
                      "gather_ms": stat(ta), "radiance_ms": stat(tb), "paths_per_s_gather": round(n*samples/np.median(ta)*1e3),
                      "paths_per_s_radiance": round(n*samples/np.median(tb)*1e3), "largest_relative_difference": worst, "kernel_ms": kernels}))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

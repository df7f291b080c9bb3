"""Times a feature-buffer call against the beauty render of the same passes (run from the repository root, on an MI355X):

    python profiles/features_measure.py [REPEATS] [WIDTH] [PASSES]          # default 7 repeats, 1024 x 1024, 16 passes

cornell, exact arithmetic, the pack's own filter.  Per repeat, interleaved, each between two device synchronises on a host clock:
  features       HipRenderer.features into a torch tensor (the device entry: no copy to the host), all three planes
  render         the beauty render of the same passes, accumulator left on the device (render(..., readback=False))
  trace_camera   HipRenderer.trace_camera x PASSES: the first-hit frames the README used to offer as denoiser inputs (host entry: every frame
                 is copied to the host, 32 bytes a pixel)
and, in repeats of their own with kernel timing on, the features call's k_features and k_accumulate spans (tinsel_hip_kernel_times: the sums
of their launches' durations) and the render's kernels.  Medians with min .. max over the repeats, in ms.  Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tinsel_amd                       # noqa: E402
from tinsel_amd import abi              # noqa: E402

WARM = 2


def main(argv):
    repeats = int(argv[1]) if len(argv) > 1 else 7
    width = int(argv[2]) if len(argv) > 2 else 1024
    passes = int(argv[3]) if len(argv) > 3 else 16
    scene = tinsel_amd.Scene.load_pack(os.path.join("tests", "golden", "cornell.pack"))
    r = tinsel_amd.create_gpu_renderer(scene)
    cam = abi.Camera.from_buffer_copy(scene.camera)
    opt = abi.Options.from_buffer_copy(scene.options)
    opt.width = opt.height = width
    r.init(width, width)
    planes = torch.empty((3, width, width, 4), dtype=torch.float32, device="cuda")

    def clocked(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0)*1000.0

    def features():
        r.features(cam, opt, 0, passes, out=planes)

    def render():
        r.set_pass_index(0)
        r.render(cam, opt, passes=passes, readback=False)

    def trace_camera():
        for _ in range(passes):
            r.trace_camera(cam, width, width)

    for _ in range(WARM):
        features()
        render()
        r.trace_camera(cam, width, width)
    torch.cuda.synchronize()
    rows = {"features": [], "render": [], "trace_camera": [], "k_features": [], "k_accumulate": [], "render_kernels": [], "render_k_accumulate": []}
    for _ in range(repeats):
        rows["features"].append(clocked(features))
        rows["render"].append(clocked(render))
        rows["trace_camera"].append(clocked(trace_camera))
    r.enable_kernel_timing(True)
    launches = None
    for _ in range(repeats):
        features()
        t = r.kernel_times()
        launches = {k: v[0] for k, v in t.items()}
        rows["k_features"].append(t["k_features"][1])
        rows["k_accumulate"].append(t["k_accumulate"][1])
        render()
        t = r.kernel_times()
        rows["render_kernels"].append(sum(v[1] for v in t.values()))
        rows["render_k_accumulate"].append(t["k_accumulate"][1])
    r.enable_kernel_timing(False)
    host = {n: v.cpu().numpy() for n, v in zip(abi.FEATURE_NAMES, planes)}
    im = tinsel_amd.feature_images(host)
    r.close()
    stat = lambda t: {"median": round(float(np.median(t)), 4), "min": round(min(t), 4), "max": round(max(t), 4)} if t else None
    print(json.dumps({"scene": "cornell", "width": width, "height": width, "passes": passes, "repeats": repeats,
                      "library": os.environ.get("TINSEL_HIP_LIB", "in-tree"), "launches_per_features_call": launches,
                      "ms": {k: stat(v) for k, v in rows.items()},
                      "coverage_mean": float(im["coverage"].mean()), "depth_mean": float(im["depth"].mean())}))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

"""Times the denoise stage against the display stage's non-local-means pair (run from the repository root, on an MI355X):

    python profiles/denoise_measure.py [REPEATS]          # default 7 repeats

Frame 1024 x 1024: cornell rendered at 4 spp, its three feature planes, everything on the device.  Radius 2, 4 and 8.
  denoise    tinsel_hip_denoise_device with every plane, patch radius 1, the default coefficients: k_denoise_prepare + k_nlm_means +
             k_denoise, between two events on the stream, CALLS calls per pair of events
  denoise0   the same with features == 0 (the colour term alone: what the yardstick computes per tap)
  nlm        the yardstick, whose code does not change: k_nlm_means + k_nlm of tinsel_hip_present at nlm_width = radius, from
             tinsel_hip_kernel_times (k_present is left out) -- the same number of taps, one expf each, no guides, every tap from global memory
Per repeat, interleaved: denoise, denoise0, nlm.  Two warm-up rounds.  Reported per radius as medians with min .. max over the repeats, in
ms per call, and the taps per second of the median: 1024*1024*(2r + 1)^2 taps (the clipped windows at the frame's border counted whole).
Prints one JSON line."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tinsel_amd                       # noqa: E402
from tinsel_amd import abi              # noqa: E402

W = H = 1024
SPP, WARM, CALLS = 4, 2, 5
RADII = (2, 4, 8)


def main(argv):
    repeats = int(argv[1]) if len(argv) > 1 else 7
    scene = tinsel_amd.Scene.load_pack(os.path.join("tests", "golden", "cornell.pack"))
    r = tinsel_amd.create_gpu_renderer(scene)
    cam, opt = scene.camera, scene.options.copy()
    opt.width, opt.height = W, H
    r.init(W, H)
    r.render(cam, opt, passes=SPP, readback=False)
    planes = r.features(cam, opt, 0, SPP, out=torch.empty((3, H, W, 4), dtype=torch.float32, device="cuda:0"))
    out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.current_stream()

    def denoise(radius, guides):
        p = tinsel_amd.denoise_params(radius=radius, patch_radius=1)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(stream)
        for _ in range(CALLS):
            r.denoise(planes if guides else None, p, out=out)
        stop.record(stream)
        stop.synchronize()
        return start.elapsed_time(stop)/CALLS

    def nlm(radius):
        r.enable_kernel_timing(True)
        r.render(cam, opt, passes=1, readback=False)            # (a render starts a new timing record)
        for _ in range(CALLS):
            r.present(opt, radius, 200.0, readback=False)
        t = r.kernel_times()
        r.enable_kernel_timing(False)
        assert t["k_nlm"][0] == CALLS and t["k_nlm_means"][0] == CALLS
        return (t["k_nlm"][1] + t["k_nlm_means"][1])/CALLS

    rows = {radius: {"denoise": [], "denoise0": [], "nlm": []} for radius in RADII}
    for k in range(WARM + repeats):
        for radius in RADII:
            got = (denoise(radius, True), denoise(radius, False), nlm(radius))
            if k >= WARM:
                for name, ms in zip(("denoise", "denoise0", "nlm"), got):
                    rows[radius][name].append(ms)
    r.close()

    def stat(t, radius):
        med = float(np.median(t))
        return {"median_ms": round(med, 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                "gtaps_per_s": round(W*H*(2*radius + 1)**2/(med*1e-3)/1e9, 2)}

    print(json.dumps({"frame": [W, H], "spp": SPP, "repeats": repeats, "calls_per_timing": CALLS, "library": os.environ.get("TINSEL_HIP_LIB", "in-tree"),
                      "radius": {str(radius): {k: stat(v, radius) for k, v in rows[radius].items()} for radius in RADII}}))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

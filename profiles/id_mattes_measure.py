"""Times the ID-matte call against the closest existing work, the single DEPTH feature plane (run from the repository root, on an MI355X):

    python profiles/id_mattes_measure.py [REPEATS]          # default 5 repeats

Frame 1024 x 1024, 16 passes, 6 slots; scenes cornell.pack and ajax_standin_96.pack; everything on the device, one process.
  mattes     tinsel_hip_render_id_mattes_device: k_ids + k_ids_accumulate per batch, k_ids_rank, between two events on the stream
  depth      tinsel_hip_render_features_device with TINSEL_FEATURE_DEPTH on the same passes: k_features + k_accumulate per batch
Both with the pack's own filter, interleaved per repeat, two warm-up rounds, medians with min .. max in ms per call.
The accumulate step alone, cornell, Gaussian filter of width 0.75 (tiled form) and 2.5 (generic form): the gather and the ranking have no
class in tinsel_hip_kernel_times, so with kernel timing on the call is timed with events and the time of its trace kernel (k_ids, reported
under "k_features") is taken off: what is left is the seed kernel, two memsets, the gathers and the ranking.  Beside it the depth plane's
"k_accumulate" class for the same filter.  Prints one JSON line."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tinsel_amd                       # noqa: E402
from tinsel_amd import abi              # noqa: E402

W = H = 1024
PASSES, SLOTS, WARM = 16, 6, 2
SCENES = ("cornell", "ajax_standin_96")
WIDTHS = (0.75, 2.5)


def main(argv):
    repeats = int(argv[1]) if len(argv) > 1 else 5
    stream = torch.cuda.current_stream()
    ids = torch.empty((SLOTS, H, W), dtype=torch.int32, device="cuda:0")
    weights = torch.empty((SLOTS + 2, H, W), dtype=torch.float32, device="cuda:0")
    plane = torch.empty((1, H, W, 4), dtype=torch.float32, device="cuda:0")

    def timed(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(stream)
        fn()
        stop.record(stream)
        stop.synchronize()
        return start.elapsed_time(stop)

    def stat(t):
        return {"median_ms": round(float(np.median(t)), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}

    result = {"frame": [W, H], "passes": PASSES, "slots": SLOTS, "repeats": repeats, "scenes": {}, "accumulate_alone": {}}
    for name in SCENES:
        scene = tinsel_amd.Scene.load_pack(os.path.join("tests", "golden", name + ".pack"))
        r = tinsel_amd.create_gpu_renderer(scene)
        cam, opt = scene.camera, scene.options.copy()
        opt.width, opt.height = W, H
        r.init(W, H)
        mattes = lambda o=opt: r.id_mattes(cam, o, 0, PASSES, SLOTS, out=(ids, weights))
        depth = lambda o=opt: r.features(cam, o, 0, PASSES, which=("depth",), out=plane)
        rows = {"mattes": [], "depth": []}
        for k in range(WARM + repeats):
            got = (timed(mattes), timed(depth))
            if k >= WARM:
                rows["mattes"].append(got[0])
                rows["depth"].append(got[1])
        result["scenes"][name] = {"filter_width": float(opt.filter.width), **{k: stat(v) for k, v in rows.items()}}

        if name == "cornell":
            r.enable_kernel_timing(True)
            for fw in WIDTHS:
                o = opt.copy()
                o.filter.type, o.filter.width, o.filter.falloff = abi.FILTER_GAUSSIAN, fw, 1.0
                o.filter.offset = float(np.exp(np.float32(-fw*fw)))
                rows = {"mattes_call": [], "k_ids": [], "mattes_rest": [], "depth_k_accumulate": [], "depth_k_features": []}
                for k in range(WARM + repeats):
                    call = timed(lambda: mattes(o))
                    t = r.kernel_times()
                    timed(lambda: depth(o))
                    d = r.kernel_times()
                    if k >= WARM:
                        rows["mattes_call"].append(call)
                        rows["k_ids"].append(t["k_features"][1])
                        rows["mattes_rest"].append(call - t["k_features"][1])
                        rows["depth_k_accumulate"].append(d["k_accumulate"][1])
                        rows["depth_k_features"].append(d["k_features"][1])
                window = 1 + int(np.floor(fw)) + int(np.ceil(fw)) + 1
                result["accumulate_alone"][str(fw)] = {"form": "tiled" if window <= 6 else "generic", "window": window, **{k: stat(v) for k, v in rows.items()}}
            r.enable_kernel_timing(False)
        r.close()
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

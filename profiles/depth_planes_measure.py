"""Times a depth-planes call against the renders it replaces (run from the repository root, on an MI355X):

    python profiles/depth_planes_measure.py measure [REPEATS] [WIDTH] [PASSES]  > measure.json
    python profiles/depth_planes_measure.py report measure.json [compare.txt]                   # writes profiles/depth_planes_measure.md

cornell (closed, the flat scan; a render takes the fused kernel), glass at depth 12 (media; the benchmark's override of glass.tin's 8) and
ajax_standin_96 (a mesh in HBM: k_walk) at their packs' own options otherwise, exact arithmetic, default 256 x 256, 16 passes, 9 repeats
after a warm-up round, each between two device synchronises on a host clock; every output stays on the device.  D is the scene's depth.
  planes 1..D     HipRenderer.depth_planes, depths 1 .. D, into a torch tensor: one k_views_accumulate launch per batch
  planes singly   the same with singly=True: one launch of the render's accumulate kernels per plane and batch -- the other accumulate choice
  planes {1, D}   depths [1, D]: direct light and the beauty
  loop 1..D       D times { set_pass_index(0); tinsel_hip_render at max_depth = d }: what the planes cost before this call (the yardstick;
                  the pipeline is the renderer's own choice, the fused kernel where the scene allows it)
  render D        one tinsel_hip_render at max_depth = D: the beauty alone (the other yardstick)
  groups G = 1    HipRenderer.light_groups with every emitter and the sky in one group: the split pipeline to depth D without planes
`report` puts the medians (min .. max), the ratios against the two yardsticks and k_shade_depths' resource line beside k_shade's
(tinsel_amd/csrc/_obj/resources.json, what build() recorded with -Rpass-analysis=kernel-resource-usage) into the .md."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARM = 1
SCENES = [("cornell", None), ("glass", 12), ("ajax_standin_96", None)]
LEGS = ["planes 1..D", "planes singly", "planes {1, D}", "loop 1..D", "render D", "groups G = 1"]


def stat(t):
    return {"median": round(float(np.median(t)), 4), "min": round(min(t), 4), "max": round(max(t), 4)}


def measure_scene(name, depth, repeats, width, passes):
    import torch
    import tinsel_amd
    from tinsel_amd import abi
    scene = tinsel_amd.Scene.load_pack(os.path.join(ROOT, "tests", "golden", name + ".pack"))
    r = tinsel_amd.create_gpu_renderer(scene)
    cam = abi.Camera.from_buffer_copy(scene.camera)
    opt = abi.Options.from_buffer_copy(scene.options)
    opt.width = opt.height = width
    if depth:
        opt.max_depth = depth
    D = int(opt.max_depth)
    assert 2 <= D <= abi.MAX_DEPTH_PLANES
    r.init(width, width)
    every = list(range(1, D + 1))
    at = []
    for d in every:
        o = opt.copy()
        o.max_depth = d
        at.append(o)
    planes = torch.empty((D, width, width, 4), dtype=torch.float32, device="cuda")
    table, env = np.zeros(scene.num_primitives, np.int32), 0
    one = torch.empty((1, width, width, 4), dtype=torch.float32, device="cuda")

    def loop():
        for o in at:
            r.set_pass_index(0)
            r.render(cam, o, passes=passes, readback=False)

    def render():
        r.set_pass_index(0)
        r.render(cam, opt, passes=passes, readback=False)

    legs = {
        "planes 1..D": lambda: r.depth_planes(cam, opt, 0, passes, every, out=planes),
        "planes singly": lambda: r.depth_planes(cam, opt, 0, passes, every, out=planes, singly=True),
        "planes {1, D}": lambda: r.depth_planes(cam, opt, 0, passes, [1, D], out=planes[:2]),
        "loop 1..D": loop,
        "render D": render,
        "groups G = 1": lambda: r.light_groups(cam, opt, 0, passes, table, env, out=one),
    }

    def clocked(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0)*1000.0

    out = {"scene": name, "depth": D, "ms": {}, "kernel_ms": {}, "launches": {}}
    for leg in LEGS:
        for _ in range(WARM):
            legs[leg]()
        torch.cuda.synchronize()
        out["ms"][leg] = stat([clocked(legs[leg]) for _ in range(repeats)])
    # the kernel spans of the two calls that differ in their shading kernel alone
    r.enable_kernel_timing(True)
    for leg in ("planes 1..D", "groups G = 1"):
        spans = {}
        for _ in range(repeats):
            legs[leg]()
            torch.cuda.synchronize()
            times = r.kernel_times()
            for k, v in times.items():
                spans.setdefault(k, []).append(v[1])
        out["kernel_ms"][leg] = {k: stat(v) for k, v in sorted(spans.items())}
        out["launches"][leg] = {k: v[0] for k, v in times.items()}
    r.close()
    return out


def report(path):
    m = json.loads(open(path).read().strip().splitlines()[-1])
    cell = lambda s: "%.3f (%.3f .. %.3f)" % (s["median"], s["min"], s["max"])
    lines = ["# Depth planes: one trace against one render per depth", "",
             "%d x %d, %d passes, MI355X, %d repeats after %d warm-up round; wall clock between two device synchronises, median (min .. max) "
             "in ms; every output stays on the device.  D is the scene's depth (glass: the benchmark's 12).  Made by "
             "`profiles/depth_planes_measure.py`, whose head says what each leg is." % (m["width"], m["width"], m["passes"], m["repeats"], WARM), "",
             "| leg | " + " | ".join("%s, D = %d" % (s["scene"], s["depth"]) for s in m["scenes"]) + " |", "|---|" + "---|"*len(m["scenes"])]
    for leg in LEGS:
        lines.append("| %s | %s |" % (leg, " | ".join(cell(s["ms"][leg]) for s in m["scenes"])))
    ratio = lambda a, b: " | ".join("%.2f" % (s["ms"][a]["median"]/s["ms"][b]["median"]) for s in m["scenes"])
    lines += ["| planes 1..D / loop 1..D | %s |" % ratio("planes 1..D", "loop 1..D"),
              "| planes 1..D / render D | %s |" % ratio("planes 1..D", "render D"),
              "| planes 1..D / groups G = 1 | %s |" % ratio("planes 1..D", "groups G = 1"),
              "| planes singly / planes 1..D | %s |" % ratio("planes singly", "planes 1..D"), ""]
    for s in m["scenes"]:
        a, b = s["kernel_ms"]["planes 1..D"], s["kernel_ms"]["groups G = 1"]
        la, lb = s["launches"]["planes 1..D"], s["launches"]["groups G = 1"]
        lines += ["Kernel spans per call on %s (sum of the launches' durations, median ms; launches in brackets):" % s["scene"], "",
                  "| kernel | planes 1..D | groups G = 1 |", "|---|---|---|"]
        for k in sorted(set(a) | set(b)):
            c = lambda t, l: "%.4f [%d]" % (t[k]["median"], l.get(k, 0)) if k in t else "-"
            lines.append("| %s | %s | %s |" % (k + (" (k_shade_depths / k_shade_groups)" if k == "k_shade" else ""), c(a, la), c(b, lb)))
        lines.append("")
    res = os.path.join(ROOT, "tinsel_amd", "csrc", "_obj", "resources.json")
    if os.path.exists(res):
        k = json.load(open(res))["kernels"]
        lines += ["Resources (`-Rpass-analysis=kernel-resource-usage`, `TN_WAVES_SHADE` = 4):", "",
                  "| kernel | VGPRs | scratch bytes/lane | SGPR spills | waves/SIMD | code bytes |", "|---|---|---|---|---|---|"]
        for n in sorted(k):
            if n.startswith("k_shade<") or n.startswith("k_shade_depths<"):
                lines.append("| %s | %d | %d | %d | %d | %d |" % (n, k[n]["vgprs"], k[n]["scratch_bytes"], k[n]["sgpr_spills"], k[n]["waves_per_simd"],
                                                                  k[n].get("code_bytes", 0)))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "report":
        text = report(sys.argv[2])
        if len(sys.argv) > 3:           # what profiles/compare_code_objects.py PARENT_TREE THIS_TREE printed
            text += "\nThe kernels that existed before (`profiles/compare_code_objects.py` against the parent commit's tree):\n\n```\n%s```\n" % open(sys.argv[3]).read()
        with open(os.path.join(ROOT, "profiles", "depth_planes_measure.md"), "w") as f:
            f.write(text)
        print(text)
        sys.exit(0)
    if len(sys.argv) < 2 or sys.argv[1] != "measure":
        raise SystemExit(__doc__)
    a = sys.argv[2:]
    repeats, width, passes = int(a[0]) if a else 9, int(a[1]) if len(a) > 1 else 256, int(a[2]) if len(a) > 2 else 16
    print(json.dumps({"repeats": repeats, "width": width, "passes": passes,
                      "scenes": [measure_scene(name, depth, repeats, width, passes) for name, depth in SCENES]}))

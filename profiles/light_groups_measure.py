"""Times a light-groups call against G renders of the same passes (run from the repository root, on an MI355X):

    python profiles/light_groups_measure.py call   [REPEATS] [WIDTH] [PASSES]  > call.json      # this tree's library
    TINSEL_HIP_LIB=PARENT/libtinsel_hip.so \\
    python profiles/light_groups_measure.py render [REPEATS] [WIDTH] [PASSES]  > render.json    # the parent commit's library
    python profiles/light_groups_measure.py report call.json render.json [compare.txt]         # writes profiles/light_groups_measure.md

veach (four lights: G = 4, one group per light), exact arithmetic, the pack's own options, default 256 x 256, 16 passes, 9 repeats after 3
warm-up rounds, each between two device synchronises on a host clock:
  call     HipRenderer.light_groups into a torch tensor (the device entry: no copy to the host)
  render   tinsel_hip_render of the same passes with the split pipeline forced, accumulator left on the device: what ONE masked scene
           costs today, so the alternative to the call is G of these
and, in repeats of their own with kernel timing on, each leg's kernel spans (tinsel_hip_kernel_times).  Medians with min .. max, in ms.
`report` puts both legs, the ratio call / (G x render) and k_shade_groups' resource line beside k_shade's (tinsel_amd/csrc/_obj/
resources.json, what build() recorded with -Rpass-analysis=kernel-resource-usage) into the .md."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARM = 3
GROUPS = [5, 6, 7, 8]


def stat(t):
    return {"median": round(float(np.median(t)), 4), "min": round(min(t), 4), "max": round(max(t), 4)}


def measure(mode, repeats, width, passes):
    import torch
    import tinsel_amd
    from tinsel_amd import abi
    scene = tinsel_amd.Scene.load_pack(os.path.join(ROOT, "tests", "golden", "veach.pack"))
    r = tinsel_amd.create_gpu_renderer(scene)
    cam = abi.Camera.from_buffer_copy(scene.camera)
    opt = abi.Options.from_buffer_copy(scene.options)
    opt.width = opt.height = width
    r.init(width, width)
    if mode == "call":
        table = np.full(scene.num_primitives, -1, np.int32)
        table[GROUPS] = np.arange(len(GROUPS))
        planes = torch.empty((len(GROUPS), width, width, 4), dtype=torch.float32, device="cuda")
        run = lambda: r.light_groups(cam, opt, 0, passes, table, out=planes)
    else:
        r.set_pipeline(abi.PIPELINE_WAVEFRONT_SPLIT)

        def run():
            r.set_pass_index(0)
            r.render(cam, opt, passes=passes, readback=False)

    def clocked(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0)*1000.0

    for _ in range(WARM):
        run()
    torch.cuda.synchronize()
    wall = [clocked(run) for _ in range(repeats)]
    r.enable_kernel_timing(True)
    kernels = {}
    for _ in range(repeats):
        run()
        torch.cuda.synchronize()
        for k, v in r.kernel_times().items():
            kernels.setdefault(k, []).append(v[1])
        launches = {k: v[0] for k, v in r.kernel_times().items()}
    r.close()
    return {"mode": mode, "scene": "veach", "groups": len(GROUPS), "width": width, "height": width, "passes": passes, "repeats": repeats,
            "library": os.environ.get("TINSEL_HIP_LIB", "in-tree"), "ms": stat(wall), "kernel_ms": {k: stat(v) for k, v in sorted(kernels.items())},
            "launches": launches}


def report(call_path, render_path):
    call, render = (json.loads(open(p).read().strip().splitlines()[-1]) for p in (call_path, render_path))
    assert call["mode"] == "call" and render["mode"] == "render" and all(call[k] == render[k] for k in ("width", "passes", "scene"))
    G = call["groups"]
    ratio = call["ms"]["median"]/(G*render["ms"]["median"])
    lines = ["# Light groups: one call against G renders", "",
             "%s at %d x %d, %d passes, G = %d (one group per light), MI355X, %d repeats after %d warm-up rounds; wall clock between two device "
             "synchronises, median (min .. max) in ms.  Made by `profiles/light_groups_measure.py`." % (
                 call["scene"], call["width"], call["height"], call["passes"], G, call["repeats"], WARM), "",
             "| leg | library | ms |", "|---|---|---|"]
    for leg, what in ((call, "`light_groups`, device entry, G = %d" % G), (render, "`tinsel_hip_render`, split pipeline forced (one masked scene)")):
        lines.append("| %s | %s | %.4f (%.4f .. %.4f) |" % (what, "this tree" if leg["library"] == "in-tree" else "parent commit", leg["ms"]["median"],
                                                          leg["ms"]["min"], leg["ms"]["max"]))
    lines += ["", "call / (G x render) = %.4f / (%d x %.4f) = **%.3f**: the call takes %s time than rendering the %d masked scenes." % (
        call["ms"]["median"], G, render["ms"]["median"], ratio, "less" if ratio < 1 else "MORE", G), "",
        "Kernel spans per call (sum of the launches' durations, median ms; launches in brackets):", "",
        "| kernel | light_groups | render |", "|---|---|---|"]
    for k in sorted(set(call["kernel_ms"]) | set(render["kernel_ms"])):
        cell = lambda leg: "%.4f [%d]" % (leg["kernel_ms"][k]["median"], leg["launches"].get(k, 0)) if k in leg["kernel_ms"] else "-"
        lines.append("| %s | %s | %s |" % (k + (" (k_shade_groups in the call)" if k == "k_shade" else ""), cell(call), cell(render)))
    res = os.path.join(ROOT, "tinsel_amd", "csrc", "_obj", "resources.json")
    if os.path.exists(res):
        k = json.load(open(res))["kernels"]
        lines += ["", "Resources (`-Rpass-analysis=kernel-resource-usage`, `TN_WAVES_SHADE` = 4):", "",
                  "| kernel | VGPRs | scratch bytes/lane | SGPR spills | waves/SIMD | code bytes |", "|---|---|---|---|---|---|"]
        for n in sorted(k):
            if n.startswith("k_shade<") or n.startswith("k_shade_groups<"):
                lines.append("| %s | %d | %d | %d | %d | %d |" % (n, k[n]["vgprs"], k[n]["scratch_bytes"], k[n]["sgpr_spills"], k[n]["waves_per_simd"],
                                                                  k[n].get("code_bytes", 0)))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "report":
        text = report(sys.argv[2], sys.argv[3])
        if len(sys.argv) > 4:           # what profiles/compare_code_objects.py PARENT_TREE THIS_TREE printed
            text += "\nThe kernels that existed before (`profiles/compare_code_objects.py` against the parent commit's tree):\n\n```\n%s```\n" % open(sys.argv[4]).read()
        with open(os.path.join(ROOT, "profiles", "light_groups_measure.md"), "w") as f:
            f.write(text)
        print(text)
        sys.exit(0)
    if len(sys.argv) < 2 or sys.argv[1] not in ("call", "render"):
        raise SystemExit(__doc__)
    a = sys.argv[2:]
    print(json.dumps(measure(sys.argv[1], int(a[0]) if a else 9, int(a[1]) if len(a) > 1 else 256, int(a[2]) if len(a) > 2 else 16)))

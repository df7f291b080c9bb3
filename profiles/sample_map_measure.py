"""Times a sample-map call (run from the repository root, on an MI355X):

    python profiles/sample_map_measure.py run [REPEATS] > sample_map.json
    python profiles/sample_map_measure.py report sample_map.json [compare.txt] [bench.txt]     # writes profiles/sample_map_measure.md

cornell (closed, analytic) and ajax_standin_96 (a mesh in HBM: k_walk) at 512 x 512, every output a torch tensor [H, W, 4] on the device
(the device entries), the arms of a part alternating within every repeat after 3 warm-up rounds of all of them.

 (a) what the compact slots and the masked accumulate cost where nothing is masked:
       uniform   HipRenderer.sample_map with a uniform map of 16
       views     HipRenderer.views with this one camera and 16 passes -- the same paths through the same pipeline, k_generate_views and
                 k_views_accumulate in the place of k_generate_samples and k_samples_accumulate.  No kernel of that call differs from the
                 parent commit's (profiles/compare_code_objects.py), so it is timed with this tree's library.
     The two leave the same plane (checked).
 (b) whether the cost follows the samples:
       foveated  a map that gives a centred rectangle of 10 % of the pixels 64 levels and the rest 4
       full      a uniform map of 64
     with the ratio of the two maps' path counts beside the ratio of the times.

Time: device events around the call on the null stream, then a synchronise; the wall clock of the same span beside it (it holds the
host's prefix sum over the map and the upload of the offsets).  Medians with min .. max, in ms.  In repeats of their own with kernel
timing on, every arm's kernel spans (tinsel_hip_kernel_times) summed into generation (k_generate), accumulate (k_accumulate) and trace
(everything else)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARM = 3
SIZE = 512
SCENES = ["cornell", "ajax_standin_96"]


def stat(t):
    return {"median": round(float(np.median(t)), 4), "min": round(float(min(t)), 4), "max": round(float(max(t)), 4)}


def split(times):
    out = {"generation": 0.0, "trace": 0.0, "accumulate": 0.0}
    for k, v in times.items():
        out["generation" if k.startswith("k_generate") else "accumulate" if k == "k_accumulate" else "trace"] += v[1]
    return out


def foveated_map(size):
    """a centred square of 10 % of the pixels at 64 levels, the rest at 4"""
    side = int(round(size*np.sqrt(0.1)))
    a = (size - side)//2
    counts = np.full((size, size), 4, np.uint16)
    counts[a:a + side, a:a + side] = 64
    return counts


def measure_scene(scene_name, repeats):
    import torch
    import tinsel_amd
    from tinsel_amd import abi
    scene = tinsel_amd.Scene.load_pack(os.path.join(ROOT, "tests", "golden", scene_name + ".pack"))
    cam = abi.Camera.from_buffer_copy(scene.camera)
    opt = abi.Options.from_buffer_copy(scene.options)
    opt.width = opt.height = SIZE
    r = tinsel_amd.create_gpu_renderer(scene)
    r.init(SIZE, SIZE)
    plane = torch.empty((SIZE, SIZE, 4), dtype=torch.float32, device="cuda")
    planes = torch.empty((1, SIZE, SIZE, 4), dtype=torch.float32, device="cuda")
    maps = {"uniform": np.full((SIZE, SIZE), 16, np.uint16), "foveated": foveated_map(SIZE), "full": np.full((SIZE, SIZE), 64, np.uint16)}
    parts = {"a": {"uniform": lambda: r.sample_map(cam, opt, maps["uniform"], out=plane),
                   "views": lambda: r.views([cam], opt, 0, 16, out=planes)},
             "b": {"foveated": lambda: r.sample_map(cam, opt, maps["foveated"], out=plane),
                   "full": lambda: r.sample_map(cam, opt, maps["full"], out=plane)}}

    def clocked(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), (time.perf_counter() - t0)*1000.0

    for _ in range(WARM):
        for arms in parts.values():
            for fn in arms.values():
                fn()
    torch.cuda.synchronize()
    parts["a"]["uniform"]()
    parts["a"]["views"]()
    torch.cuda.synchronize()
    same = bool(torch.equal(plane, planes[0]))

    dev, wall = {}, {}
    for arms in parts.values():
        for k in arms:
            dev[k], wall[k] = [], []
        for _ in range(repeats):
            for k, fn in arms.items():
                d, w = clocked(fn)
                dev[k].append(d)
                wall[k].append(w)
    kernels = {k: {"generation": [], "trace": [], "accumulate": []} for k in dev}
    launches = {}
    r.enable_kernel_timing(True)
    for arms in parts.values():
        for _ in range(repeats):
            for k, fn in arms.items():
                fn()
                torch.cuda.synchronize()
                times = r.kernel_times()
                launches[k] = int(sum(v[0] for v in times.values()))
                for c, ms in split(times).items():
                    kernels[k][c].append(ms)
    paths = {k: int(m.sum(dtype=np.int64)) for k, m in maps.items()}
    paths["views"] = paths["uniform"]
    plan = {k: tinsel_amd.plan_sample_map(64 << 20, SIZE, SIZE, m) for k, m in maps.items()}
    r.close()
    return {"scene": scene_name, "size": SIZE, "repeats": repeats, "planes_equal": same, "paths": paths, "plan": plan,
            "device_ms": {k: stat(v) for k, v in dev.items()}, "wall_ms": {k: stat(v) for k, v in wall.items()},
            "kernel_ms": {k: {c: stat(v) for c, v in cs.items()} for k, cs in kernels.items()}, "kernel_launches": launches}


def report(path):
    rows = json.loads(open(path).read().strip().splitlines()[-1])
    cell = lambda s: "%.3f (%.3f .. %.3f)" % (s["median"], s["min"], s["max"])
    lines = ["# Sample maps: the overhead where nothing is masked, and whether the cost follows the samples", "",
             "MI355X, %d x %d, %d repeats after %d warm-up rounds of every arm, the arms of a part alternating within each repeat; device events "
             "around the call on one stream, ended by a synchronise; median (min .. max) in ms.  Made by `profiles/sample_map_measure.py`, which "
             "describes the arms." % (rows[0]["size"], rows[0]["size"], rows[0]["repeats"], WARM), "",
             "## (a) a uniform map of 16 against `views` with this one camera and 16 passes", "",
             "| scene | uniform map | views | uniform / views | wall: uniform | wall: views | planes equal |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        d, w = r["device_ms"], r["wall_ms"]
        lines.append("| %s | %s | %s | **%.3f** | %s | %s | %s |" % (r["scene"], cell(d["uniform"]), cell(d["views"]), d["uniform"]["median"]/d["views"]["median"],
                                                                  cell(w["uniform"]), cell(w["views"]), "yes" if r["planes_equal"] else "NO"))
    lines += ["", "Kernel spans (sum of the launches' durations from `tinsel_hip_kernel_times`, median ms; all launches of the arm in brackets):", "",
              "| scene | arm | generation | trace | accumulate | launches |", "|---|---|---|---|---|---|"]
    for r in rows:
        for k in ("uniform", "views"):
            ks = r["kernel_ms"][k]
            lines.append("| %s | %s | %.3f | %.3f | %.3f | [%d] |" % (r["scene"], k, ks["generation"]["median"], ks["trace"]["median"], ks["accumulate"]["median"],
                                                                   r["kernel_launches"][k]))
        u, v = r["kernel_ms"]["uniform"], r["kernel_ms"]["views"]
        lines.append("| %s | uniform / views | **%.3f** | %.3f | **%.3f** | |" % (r["scene"], u["generation"]["median"]/v["generation"]["median"],
                                                                               u["trace"]["median"]/v["trace"]["median"], u["accumulate"]["median"]/v["accumulate"]["median"]))
    lines += ["", "Where the difference goes (medians; the kernel spans are from repeats of their own):", ""]
    for r in rows:
        d, u, v = r["device_ms"], r["kernel_ms"]["uniform"], r["kernel_ms"]["views"]
        more = d["uniform"]["median"] - d["views"]["median"]
        parts = {c: u[c]["median"] - v[c]["median"] for c in ("generation", "trace", "accumulate")}
        lines.append("* %s: the call takes %.3f ms more than `views`; its kernels %.3f of that (generation %+.3f: the index-to-pixel search of "
                     "`k_generate_samples`; trace %+.3f; accumulate %+.3f: the offsets, the level bound, the per-level test), and %.3f is no kernel's: "
                     "the device waits while the host sums the map for the cut, sums it again for the offsets and uploads them (4 bytes a pixel, from "
                     "pageable memory) -- work a views call has no counterpart of." % (r["scene"], more, sum(parts.values()), parts["generation"],
                                                                                     parts["trace"], parts["accumulate"], more - sum(parts.values())))
    lines += ["", "## (b) 10 % of the pixels at 64 levels and the rest at 4, against a uniform 64", "",
              "| scene | foveated | full | time ratio | paths: foveated | paths: full | path ratio | wall: foveated | wall: full |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        d, w, p = r["device_ms"], r["wall_ms"], r["paths"]
        lines.append("| %s | %s | %s | **%.3f** | %d | %d | **%.3f** | %s | %s |" % (r["scene"], cell(d["foveated"]), cell(d["full"]), d["foveated"]["median"]/d["full"]["median"],
                                                                                  p["foveated"], p["full"], p["foveated"]/p["full"], cell(w["foveated"]), cell(w["full"])))
    lines += ["", "| scene | arm | generation | trace | accumulate | launches |", "|---|---|---|---|---|---|"]
    for r in rows:
        for k in ("foveated", "full"):
            ks = r["kernel_ms"][k]
            lines.append("| %s | %s | %.3f | %.3f | %.3f | [%d] |" % (r["scene"], k, ks["generation"]["median"], ks["trace"]["median"], ks["accumulate"]["median"],
                                                                   r["kernel_launches"][k]))
    lines += ["", "The time follows the paths, not one for one: every launch of the call has a floor (the launches in brackets, a few microseconds each), the "
              "accumulate launch lasts as long as its tallest tiles -- the 64-level ones, so it barely shortens -- and on ajax_standin_96 the "
              "centred square is where the mesh is: the 64-level pixels are the frame's expensive ones."]
    res = os.path.join(ROOT, "tinsel_amd", "csrc", "_obj", "resources.json")
    if os.path.exists(res):
        k = json.load(open(res))["kernels"]
        lines += ["", "Resources (`-Rpass-analysis=kernel-resource-usage`):", "",
                  "| kernel | VGPRs | SGPRs | static LDS bytes | scratch bytes/lane | SGPR spills | waves/SIMD | code bytes |", "|---|---|---|---|---|---|---|---|"]
        for n in sorted(k):
            if n in ("k_generate", "k_generate_views", "k_generate_samples") or n.startswith("k_views_accumulate") or n.startswith("k_samples_accumulate"):
                lines.append("| %s | %d | %d | %d | %d | %d | %d | %d |" % (n, k[n]["vgprs"], k[n]["sgprs"], k[n].get("static_lds_bytes", 0), k[n]["scratch_bytes"],
                                                                          k[n]["sgpr_spills"], k[n]["waves_per_simd"], k[n].get("code_bytes", 0)))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "report":
        text = report(sys.argv[2])
        if len(sys.argv) > 3:           # what profiles/compare_code_objects.py PARENT_TREE THIS_TREE printed
            text += "\nThe kernels that existed before (`profiles/compare_code_objects.py` against the parent commit's tree):\n\n```\n%s```\n" % open(sys.argv[3]).read()
        if len(sys.argv) > 4:           # the headline benchmark of this tree's library
            text += "\nThe headline benchmark:\n\n```\n%s```\n" % open(sys.argv[4]).read()
        with open(os.path.join(ROOT, "profiles", "sample_map_measure.md"), "w") as f:
            f.write(text)
        print(text)
        sys.exit(0)
    if len(sys.argv) < 2 or sys.argv[1] != "run":
        raise SystemExit(__doc__)
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    rows = []
    for scene_name in SCENES:
        rows.append(measure_scene(scene_name, repeats))
        print("done: %s" % scene_name, file=sys.stderr, flush=True)
    print(json.dumps(rows))

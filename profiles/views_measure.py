"""Times a views call against the cheapest loop over single-camera renders that leaves the same V accumulators on the device (run from the
repository root, on an MI355X):

    python profiles/views_measure.py run [REPEATS] > views.json
    python profiles/views_measure.py report views.json [compare.txt] [bench.txt]     # writes profiles/views_measure.md

Shapes: 64 views x 128 x 128 x 4 passes (a turntable, tinsel_amd.orbit_cameras about what the pack's camera sees at the centre of the
frame) and 6 views x 256 x 256 x 16 passes (a cube map, tinsel_amd.cube_cameras half-way between the camera and that point), each on
cornell (a closed scene: a render takes the fused kernel) and ajax_standin_96 (a mesh in HBM: k_walk).  Three arms, alternating within
every repeat, after 3 warm-up rounds of all three:

  views    HipRenderer.views into a torch tensor [V, H, W, 4] (the device entry, one accumulate launch per batch)
  singly   the same with singly=True (one accumulate launch of the render's own kernels per view)
  loop     the cheapest loop over the API of the commit before view batches: ONE renderer whose accumulator is a torch tensor
           (init(accum_tensor=...)), and per view  accum.zero_() ; set_pass_index(0) ; render_async(camera, passes) ; planes[v].copy_(accum)
           -- every step enqueued on the one stream, no host wait inside the loop, no copy to the host.  (init or write_accum per view
           would synchronise the device twice a view.)  It runs what AUTO picks for a render, the fused kernel on cornell.  No kernel of
           that loop differs from the parent commit's (profiles/compare_code_objects.py), so it is timed with this tree's library.

The loop has a renderer of its own: the call traces in the split or paired pipeline's path buffers and a render on cornell in the fused
kernel's, so one renderer alternating between them would re-allocate its path buffers at every switch, which no user's loop does.
Time: device events around the arm's work on the null stream, then a synchronise; the wall clock of the same span beside it.  Medians
with min .. max, in ms.  In repeats of their own with kernel timing on, every arm's kernel spans (tinsel_hip_kernel_times) summed into
generation (k_generate), accumulate (k_accumulate) and trace (everything else); the loop's are summed over its V calls."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARM = 3
SHAPES = [("turntable", 64, 128, 4), ("cube map", 6, 256, 16)]
SCENES = ["cornell", "ajax_standin_96"]


def stat(t):
    return {"median": round(float(np.median(t)), 4), "min": round(float(min(t)), 4), "max": round(float(max(t)), 4)}


def split(times):
    out = {"generation": 0.0, "trace": 0.0, "accumulate": 0.0}
    for k, v in times.items():
        out["generation" if k.startswith("k_generate") else "accumulate" if k == "k_accumulate" else "trace"] += v[1]
    return out


def measure_shape(scene_name, what, V, size, passes, repeats):
    import torch
    import tinsel_amd
    from tinsel_amd import abi
    scene = tinsel_amd.Scene.load_pack(os.path.join(ROOT, "tests", "golden", scene_name + ".pack"))
    cam = abi.Camera.from_buffer_copy(scene.camera)
    opt = abi.Options.from_buffer_copy(scene.options)
    opt.width = opt.height = size
    r = tinsel_amd.create_gpu_renderer(scene)
    r.init(size, size)
    t, primitive, _ = r.first_hit(cam, size, size)
    origin, directions = tinsel_amd.camera_rays(cam, size, size)
    j = i = size//2
    assert primitive[j, i] >= 0
    center = origin + float(t[j, i])*directions[j, i]
    cams = tinsel_amd.orbit_cameras(cam, center, V) if what == "turntable" else tinsel_amd.cube_cameras(0.5*(origin + center))
    assert len(cams) == V
    planes = torch.empty((V, size, size, 4), dtype=torch.float32, device="cuda")
    loop_planes = torch.empty_like(planes)
    accum = torch.zeros((size, size, 4), dtype=torch.float32, device="cuda")
    r2 = tinsel_amd.create_gpu_renderer(scene)
    r2.init(size, size, accum_tensor=accum)

    def loop(per_view=None):
        for v in range(V):
            accum.zero_()
            r2.set_pass_index(0)
            r2.render_async(cams[v], opt, passes)
            loop_planes[v].copy_(accum)
            if per_view:
                per_view()

    arms = {"views": lambda: r.views(cams, opt, 0, passes, out=planes),
            "singly": lambda: r.views(cams, opt, 0, passes, out=planes, singly=True),
            "loop": loop}

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
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    # the three arms leave the same planes
    arms["views"]()
    arms["loop"]()
    torch.cuda.synchronize()
    same = bool(torch.equal(planes, loop_planes))
    dev, wall = {k: [] for k in arms}, {k: [] for k in arms}
    for _ in range(repeats):
        for k, fn in arms.items():
            d, w = clocked(fn)
            dev[k].append(d)
            wall[k].append(w)
    kernels = {k: {"generation": [], "trace": [], "accumulate": []} for k in arms}
    launches = {}
    r.enable_kernel_timing(True)
    r2.enable_kernel_timing(True)
    for _ in range(repeats):
        for k in ("views", "singly"):
            arms[k]()
            torch.cuda.synchronize()
            times = r.kernel_times()
            launches[k] = int(sum(v[0] for v in times.values()))
            for c, ms in split(times).items():
                kernels[k][c].append(ms)
        total, count = {"generation": 0.0, "trace": 0.0, "accumulate": 0.0}, [0]

        def per_view():
            torch.cuda.synchronize()
            times = r2.kernel_times()
            count[0] += int(sum(v[0] for v in times.values()))
            for c, ms in split(times).items():
                total[c] += ms
        loop(per_view)
        launches["loop"] = count[0]
        for c, ms in total.items():
            kernels["loop"][c].append(ms)
    plan = tinsel_amd.plan_views(64 << 20, size, size, passes, V)
    r.close()
    r2.close()
    return {"scene": scene_name, "shape": what, "views": V, "width": size, "height": size, "passes": passes, "repeats": repeats, "plan": plan,
            "planes_equal": same, "device_ms": {k: stat(v) for k, v in dev.items()}, "wall_ms": {k: stat(v) for k, v in wall.items()},
            "kernel_ms": {k: {c: stat(v) for c, v in cs.items()} for k, cs in kernels.items()}, "kernel_launches": launches}


def report(path):
    rows = json.loads(open(path).read().strip().splitlines()[-1])
    cell = lambda s: "%.3f (%.3f .. %.3f)" % (s["median"], s["min"], s["max"])
    lines = ["# View batches: one call against a loop of renders", "",
             "MI355X, %d repeats after %d warm-up rounds of every arm, the three arms alternating within each repeat; device events around the arm's "
             "work on one stream, ended by a synchronise; median (min .. max) in ms.  Made by `profiles/views_measure.py`, which describes the "
             "arms: `views` is the call with one accumulate launch per batch, `singly` the call with one per view, `loop` the cheapest loop over "
             "the API before view batches that leaves the same planes on the device (accumulator in a tensor; per view zero it, "
             "`set_pass_index`, `render_async`, copy the plane; nothing waited for)." % (rows[0]["repeats"], WARM), "",
             "| scene | shape | views | singly | loop | views / loop | views / singly | planes equal |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        d = r["device_ms"]
        lines.append("| %s | %d x %d x %d x %d passes (%s) | %s | %s | %s | **%.3f** | **%.3f** | %s |" % (
            r["scene"], r["views"], r["width"], r["height"], r["passes"], r["shape"], cell(d["views"]), cell(d["singly"]), cell(d["loop"]),
            d["views"]["median"]/d["loop"]["median"], d["views"]["median"]/d["singly"]["median"], "yes" if r["planes_equal"] else "NO"))
    lines += ["", "Wall clock of the same spans (host clock between two device synchronises):", "",
              "| scene | shape | views | singly | loop |", "|---|---|---|---|---|"]
    for r in rows:
        w = r["wall_ms"]
        lines.append("| %s | %s | %s | %s | %s |" % (r["scene"], r["shape"], cell(w["views"]), cell(w["singly"]), cell(w["loop"])))
    lines += ["", "Kernel spans per arm (sum of the launches' durations from `tinsel_hip_kernel_times`, median ms; the loop's summed over its V "
              "calls; all launches of the arm in brackets):", "",
              "| scene | shape | arm | generation | trace | accumulate | launches |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        for k in ("views", "singly", "loop"):
            ks = r["kernel_ms"][k]
            lines.append("| %s | %s | %s | %.3f | %.3f | %.3f | [%d] |" % (r["scene"], r["shape"], k, ks["generation"]["median"], ks["trace"]["median"],
                                                                        ks["accumulate"]["median"], r["kernel_launches"][k]))
    res = os.path.join(ROOT, "tinsel_amd", "csrc", "_obj", "resources.json")
    if os.path.exists(res):
        k = json.load(open(res))["kernels"]
        lines += ["", "Resources (`-Rpass-analysis=kernel-resource-usage`):", "",
                  "| kernel | VGPRs | SGPRs | static LDS bytes | scratch bytes/lane | SGPR spills | waves/SIMD | code bytes |", "|---|---|---|---|---|---|---|---|"]
        for n in sorted(k):
            if n in ("k_generate", "k_generate_views", "k_accumulate_tiled<0,256,0>", "k_accumulate_tiled<3,256,0>", "k_accumulate_tiled<4,256,0>") or n.startswith("k_views_accumulate"):
                lines.append("| %s | %d | %d | %d | %d | %d | %d | %d |" % (n, k[n]["vgprs"], k[n]["sgprs"], k[n].get("static_lds_bytes", 0), k[n]["scratch_bytes"],
                                                                          k[n]["sgpr_spills"], k[n]["waves_per_simd"], k[n].get("code_bytes", 0)))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "report":
        text = report(sys.argv[2])
        if len(sys.argv) > 3:           # what profiles/compare_code_objects.py PARENT_TREE THIS_TREE printed
            text += "\nThe kernels that existed before (`profiles/compare_code_objects.py` against the parent commit's tree):\n\n```\n%s```\n" % open(sys.argv[3]).read()
        if len(sys.argv) > 4:           # the headline benchmark of this tree's and the parent commit's library, alternating
            text += "\nThe headline benchmark, this tree's library and the parent commit's alternating:\n\n```\n%s```\n" % open(sys.argv[4]).read()
        with open(os.path.join(ROOT, "profiles", "views_measure.md"), "w") as f:
            f.write(text)
        print(text)
        sys.exit(0)
    if len(sys.argv) < 2 or sys.argv[1] != "run":
        raise SystemExit(__doc__)
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    rows = []
    for scene_name in SCENES:
        for what, V, size, passes in SHAPES:
            rows.append(measure_shape(scene_name, what, V, size, passes, repeats))
            print("done: %s %s" % (scene_name, what), file=sys.stderr, flush=True)
    print(json.dumps(rows))

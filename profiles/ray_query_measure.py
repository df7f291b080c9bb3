"""Times k_query and k_normals through tinsel_hip_kernel_times, one kernel per process (run it once per number, from the repository root):

    python profiles/ray_query_measure.py camera  SCENE WIDTH HEIGHT      # k_query, camera mode (tinsel_hip_trace_camera)
    python profiles/ray_query_measure.py normals SCENE WIDTH HEIGHT      # k_normals (TINSEL_MODE_NORMALS)
    python profiles/ray_query_measure.py rays    SCENE LOG2_N [occluded] [noflat]   # k_query on 2^LOG2_N incoherent rays (device entry)
                                          # noflat: the renderer is created with Tuning(flat_scan=0) -- the scene takes the scene BVH walk,
                                          # and plan_query sends its queries to k_query_refill: the ray-replacement arm on a flat-scan scene
    python profiles/ray_query_measure.py copy                            # tinsel_hip_ubench's stream copy, 256 MiB

Each run: 5 warm-up launches, then 20 timed ones; prints one JSON line (ms: min, median, max).  The incoherent rays: seed 1, origins
uniform in the bounded primitives' box grown by half its size, directions uniform on the sphere, time uniform in [0, 1], tmax = +inf.
Lanes active: the same `rays` command under `rocprofv3 --pmc SQ_INSTS_VALU SQ_THREAD_CYCLES_VALU -d DIR --output-format csv --`, in a run of
its own; SQ_THREAD_CYCLES_VALU / (64 SQ_INSTS_VALU) over the k_query dispatches.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tinsel_amd                       # noqa: E402
from tinsel_amd import abi              # noqa: E402

WARM, TIMED = 5, 20


def incoherent_rays(scene, n, seed=1):
    prims = C.cast(scene.desc.primitives, C.POINTER(abi.Primitive))
    nodes = C.cast(scene.desc.bvh_nodes, C.POINTER(abi.BVHNode))
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for k in range(scene.desc.num_bvh_nodes):          # the leaf boxes of the scene BVH that are not a plane's
        nd = nodes[k]
        if nd.right_index_leaf >> 31 and prims[nd.left_index].type != abi.GEOM_PLANE:
            lo, hi = np.minimum(lo, list(nd.lower)), np.maximum(hi, list(nd.upper))
    rng = np.random.default_rng(seed)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3] = lo - 0.5*(hi - lo) + rng.random((n, 3))*2.0*(hi - lo)
    rays[:, 3] = rng.random(n)
    v = rng.normal(size=(n, 3))
    rays[:, 4:7] = v/np.linalg.norm(v, axis=1, keepdims=True)
    rays[:, 7] = np.inf
    return rays


def main(argv):
    what = argv[1]
    if what == "copy":
        ms, units = tinsel_amd.renderer.ubench(0, 256 << 20)
        print(json.dumps({"what": "copy", "ms": ms, "GBps": units/ms/1e6}))
        return 0
    scene = tinsel_amd.Scene.load_pack(os.path.join("tests", "golden", argv[2] + ".pack"))
    noflat = "noflat" in argv[3:]
    r = tinsel_amd.HipRenderer(scene, 0, abi.Tuning(flat_scan=0)) if noflat else tinsel_amd.create_gpu_renderer(scene)
    r.enable_kernel_timing(True)
    cam, opt = abi.Camera.from_buffer_copy(scene.camera), abi.Options.from_buffer_copy(scene.options)
    out = {"what": what, "scene": argv[2], "flat_scan": 0 if noflat else -1}
    if what in ("camera", "normals"):
        W, H = int(argv[3]), int(argv[4])
        opt.width, opt.height, opt.mode = W, H, abi.MODE_NORMALS
        r.init(W, H)
        kernel = "k_query" if what == "camera" else "k_normals"
        step = (lambda: r.trace_camera(cam, W, H)) if what == "camera" else (lambda: r.render(cam, opt, passes=1, readback=False))
        out["frame"] = [W, H]
        rays_per_launch = W*H
    else:
        import torch
        n = 1 << int(argv[3])
        mode = "occluded" if "occluded" in argv[4:] else "closest"
        d = torch.from_numpy(incoherent_rays(scene, n)).cuda()
        kernel = "k_query"


        def step():
            r.trace_rays(d, mode)
            torch.cuda.synchronize()
        out["rays"], out["mode"] = n, mode
        rays_per_launch = n
    ms = []
    for k in range(WARM + TIMED):
        step()
        launches, total, _ = r.kernel_times()[kernel]
        if k >= WARM:
            ms.append(total)            # (a call's launches together)
            out["launches_per_call"] = launches
    r.close()
    ms.sort()
    out.update(kernel=kernel, ms_min=ms[0], ms_median=ms[len(ms)//2], ms_max=ms[-1], mrays_s_best=rays_per_launch/ms[0]/1e3)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

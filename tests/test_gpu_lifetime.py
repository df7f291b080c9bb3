"""Nothing is lost across a renderer's life: whatever a renderer (or a group) allocates goes back when it is destroyed.

A CHILD process (so that other tests' allocations do not move the number) runs the same cycle N = 8 times -- create, init, render,
a second init at another size, look-ahead renders, present with NLM, render_cost, a host ray query in each mode, set_mesh_bvh(PLOC)
and back, set_tuning, destroy; then a group of two members through init / look-ahead render / present / destroy -- and reports the
device's free memory after cycle 1 and after cycle N.  Every call succeeds: nothing is provoked.

The slack is twice the largest fall the same child shows against the parent commit's library, which frees everything on this path by
hand: three runs per scene in one GPU visit, beside three of this tree (profiles/r08_host_owners.md).  The parent's fall was 0 B in all
six runs (the runtime's own pools have settled by the end of cycle 1), and so was this tree's; twice 0 is 0."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CYCLES = 8
SLACK_BYTES = 2*0


def _cycle(name):
    from tinsel_amd import HipRendererGroup, abi, create_gpu_renderer
    from tests.test_gpu_parity import _load
    scene, cam, opt, _ = _load(name)
    small = opt.copy()
    small.width, small.height = opt.width//2, opt.height//2

    r = create_gpu_renderer(scene)
    r.init(opt.width, opt.height)
    r.render(cam, opt, passes=2)
    r.init(small.width, small.height)
    r.set_lookahead(abi.LOOKAHEAD_ON)
    for _ in range(3):
        r.render(cam, small, passes=1)
    r.present(small, nlm_width=1, nlm_falloff=200.0)
    r.render_cost(cam, small, 0, 1)
    rng = np.random.default_rng(7)
    rays = np.zeros((4096, 8), np.float32)
    rays[:, 0:3] = rng.uniform(-1.0, 1.0, (4096, 3)) + np.array([0.0, 1.0, 0.0])
    rays[:, 3] = 0.5
    d = rng.normal(size=(4096, 3))
    rays[:, 4:7] = d/np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 7] = 1e30
    r.trace_rays(rays, "closest")
    r.trace_rays(rays, "occluded")
    r.set_mesh_bvh(abi.BVH_PLOC)
    r.set_mesh_bvh(abi.BVH_REFERENCE)
    r.set_tuning(grid_mult=16)
    r.close()

    grp = HipRendererGroup(scene, 2, 32)
    grp.init(small.width, small.height)
    grp.set_lookahead(abi.LOOKAHEAD_ON)
    for _ in range(3):
        grp.render(cam, small, passes=1)
    grp.present(small, nlm_width=1, nlm_falloff=200.0)
    grp.close()


def _child(name):
    import torch
    free = []
    for k in range(CYCLES):
        _cycle(name)
        if k == 0 or k == CYCLES - 1:
            torch.cuda.synchronize()
            free.append(int(torch.cuda.mem_get_info()[0]))
    print("LIFETIME " + json.dumps({"scene": name, "free_after_first": free[0], "free_after_last": free[1], "fall": free[0] - free[1]}))


def run_child(name, lib=None):
    """the child's report; `lib`: another build of the library (TINSEL_HIP_LIB) for the comparison in profiles/r08_host_owners.md"""
    env = dict(os.environ, TINSEL_HIP_GROUP_ONE_DEVICE="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    if lib:
        env["TINSEL_HIP_LIB"] = lib
    p = subprocess.run([sys.executable, "-m", "tests.test_gpu_lifetime", name], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("LIFETIME ")][-1]
    return json.loads(line[len("LIFETIME "):])


@pytest.mark.parametrize("name", ["cornell", "glass"])
def test_free_memory_does_not_fall_over_renderer_lives(name):
    rep = run_child(name)
    print(rep)
    assert rep["fall"] <= SLACK_BYTES, rep


if __name__ == "__main__":
    _child(sys.argv[1])

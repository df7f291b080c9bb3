"""bench.py's plain run: exactly K timed steps after W warm-up steps, and --dump-outputs writes what those steps computed -- the
accumulator a caller of the timed path receives -- so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_k_steps_and_dumps_them(tmp_path):
    steps, warmup, w, h = 6, 2, 320, 240
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--width", str(w), "--height", str(h), "--dump-outputs", str(tmp_path)],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == warmup and d["ms_per_step"] > 0 and d["unit"] == "Msamples/s" and d["dtype"] == "f32"
    # one timed block of K passes over the frame: value x ms_per_step x K = the samples of K passes
    assert abs(d["value"]*d["ms_per_step"]*1e-3*steps*1e6 - steps*w*h) < 1e-3*steps*w*h
    # the extras are --full's: nothing of them in a plain run
    assert d["roofline"] is None and d["cpu_baseline"] is None and "configs" not in d and "detail" not in d

    got = np.load(os.path.join(tmp_path, "accum.npy"))
    assert got.dtype == np.float32 and got.shape == (h, w, 4)
    # the same K passes (pass indices [W, W + K)) rendered directly through the API
    import tinsel_amd
    from tinsel_amd import abi
    scene = tinsel_amd.Scene.load_pack(os.path.join(ROOT, "tests", "golden", "cornell.pack"))
    cam, opt = scene.camera, scene.options.copy()
    opt.width, opt.height, opt.mode = w, h, abi.MODE_PATHTRACE
    r = tinsel_amd.create_gpu_renderer(scene, 0)
    r.init(w, h)
    r.set_pass_index(warmup)
    want = r.render(cam, opt, passes=steps)
    r.close()
    assert np.allclose(got, want, rtol=1e-4, atol=1e-5), float(np.abs(got - want).max())

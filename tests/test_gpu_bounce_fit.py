"""k_bounce's FIT instances (tn_fused.h: the fused kernel compiled for a fixed set of scene and plan features) against the general kernel,
forced through tinsel_hip_tuning::bounce_fit = 0.  Every comparison is bit for bit on the accumulator; the instance that ran is read back
through tinsel_hip_bounce_plan.  (The env_loft rows need tests/golden/large/; the probe coverage that needs no large pack is
tests/test_gpu_probe_synthetic.py.)"""
import os

import numpy as np
import pytest

import tinsel_amd
from tinsel_amd import abi, create_gpu_renderer
from tinsel_amd.renderer import scene_delta
from tests.oracle_api import GOLDEN

pytestmark = pytest.mark.gpu

ENV_LOFT = os.path.join(GOLDEN, "large", "env_loft.pack")
F = abi


def _scene(name):
    path = ENV_LOFT if name == "env_loft" else os.path.join(GOLDEN, name + ".pack")
    if not os.path.exists(path):
        pytest.skip("%s not generated (tests/golden/make_probe.py)" % os.path.relpath(path, GOLDEN))
    g = np.load(os.path.join(GOLDEN, name + ".golden.npz"))
    scene = tinsel_amd.Scene.load_pack(path)
    return scene, abi.Camera.from_buffer_copy(g["camera"].tobytes()), abi.Options.from_buffer_copy(g["options"].tobytes()), g


def _render(scene, cam, opt, passes, size=None, fit=-1, r=None, **tune):
    o = opt.copy()
    if size:
        o.width, o.height = size
    own = r is None
    if own:
        r = create_gpu_renderer(scene, 0, abi.Tuning(bounce_fit=fit, **tune))
    r.init(o.width, o.height)
    r.set_pass_index(0)
    out = r.render(cam, o, passes=passes)
    plan = r.bounce_plan()
    if own:
        r.close()
    return out, plan


SCENE_MASK = F.BOUNCE_MEDIA | F.BOUNCE_PROBE | F.BOUNCE_MOTION | F.BOUNCE_MESH_WALK | F.BOUNCE_SPHERE | F.BOUNCE_TRANSMISSION

# (scene, frame, passes, tuning, the kind the plan must pick).  A batch of fewer than about two million paths is cut into regions of at
# most 512 and shares them (trace_fused), which the closed instance is not compiled for: the small cornell frames reach it with sharing
# switched off on both sides of the comparison, the 1024 x 1024 x 3 one (regions of 768) as the library plans it.
CASES = [
    ("cornell", (64, 48), 3, dict(bounce_share=0), F.BOUNCE_FIT_CLOSED),
    ("cornell", (1024, 1024), 3, {}, F.BOUNCE_FIT_CLOSED),
    ("cornell", (64, 48), 3, {}, F.BOUNCE_GENERAL),         # shared regions: the general kernel
    ("cornell", (32, 32), 16, {}, F.BOUNCE_GENERAL),        # the same (the shared instance built for it did not win and is not compiled)
    ("veach", (64, 48), 3, {}, F.BOUNCE_FIT_DEFERRED),
    ("gloss", (64, 48), 3, {}, F.BOUNCE_GENERAL),           # open, sorted queues without deferred walks: no instance
    ("env_loft", (64, 48), 3, {}, F.BOUNCE_GENERAL),        # a probe
    ("features", (64, 48), 3, {}, F.BOUNCE_GENERAL),        # media, motion, transmission, a walked mesh
]


@pytest.mark.parametrize("name,size,passes,tune,kind", CASES, ids=["%s-%dx%d%s" % (c[0], c[1][0], c[1][1], "-noshare" if c[3] else "") for c in CASES])
def test_fit_instance_against_the_general_kernel(name, size, passes, tune, kind):
    scene, cam, opt, g = _scene(name)
    out, plan = _render(scene, cam, opt, passes, size, **tune)
    ref, plan0 = _render(scene, cam, opt, passes, size, fit=0, **tune)
    assert plan0[0] == F.BOUNCE_GENERAL, plan0
    assert plan[0] == kind, plan
    assert plan[1] == plan0[1], "the features asked for do not depend on the switch"
    assert bool(plan[1] & F.BOUNCE_SHARE) == (not tune and size != (1024, 1024)), plan
    assert plan[1] & SCENE_MASK == scene.bounce_features(), plan
    assert np.isfinite(out).all() and np.array_equal(out, ref)


@pytest.mark.parametrize("name", ["cornell", "veach", "gloss", "env_loft", "features"])
def test_fit_instance_against_the_golden(name):
    scene, cam, opt, g = _scene(name)
    out, plan = _render(scene, cam, opt, int(g["passes"]))
    assert np.array_equal(out, g["accum"]), plan


def test_the_mask_follows_a_rebuilt_scene():
    """anim_cornell_0 -> 1 -> 2 -> 3 on ONE renderer (set_primitive_transform + rebuild_scene): each frame is a fresh renderer's"""
    frames = [tinsel_amd.Scene.load_pack(os.path.join(GOLDEN, "anim_cornell_%d.pack" % k)) for k in range(4)]
    cam, opt = frames[0].camera, frames[0].options.copy()
    opt.width, opt.height, opt.mode = 64, 48, abi.MODE_PATHTRACE
    r = create_gpu_renderer(frames[0])
    for k, scene in enumerate(frames):
        if k:
            moves, nodes = scene_delta(frames[k - 1], scene)
            for i, s, e in moves:
                r.set_primitive_transform(i, s, e)
            r.rebuild_scene(nodes)
        out, plan = _render(scene, cam, opt, 3, r=r)
        fresh, plan_fresh = _render(scene, cam, opt, 3)
        assert plan == plan_fresh, (k, plan, plan_fresh)
        assert np.array_equal(out, fresh), k
    r.close()


def test_the_mask_follows_roulette():
    scene, cam, opt, g = _scene("cornell")
    r = create_gpu_renderer(scene)
    r.set_tuning(bounce_share=0)            # (so that the closed instance is what roulette takes the scene away from)
    a, plan_a = _render(scene, cam, opt, 3, (64, 48), r=r)
    r.set_russian_roulette(2)
    b, plan_b = _render(scene, cam, opt, 3, (64, 48), r=r)
    r.set_russian_roulette(0)
    c, plan_c = _render(scene, cam, opt, 3, (64, 48), r=r)
    r.close()
    r0 = create_gpu_renderer(scene, 0, abi.Tuning(bounce_fit=0, bounce_share=0))
    r0.set_russian_roulette(2)
    b0, plan_b0 = _render(scene, cam, opt, 3, (64, 48), r=r0)
    r0.close()
    assert plan_a[0] == F.BOUNCE_FIT_CLOSED and plan_c == plan_a
    assert plan_b[0] == F.BOUNCE_GENERAL and plan_b[1] & F.BOUNCE_ROULETTE and plan_b0 == plan_b
    assert np.array_equal(a, c) and np.array_equal(b, b0) and not np.array_equal(a, b)


def test_the_mask_follows_the_frame_size():
    """32 x 32 x 16 passes is cut into regions of 64 paths, which a workgroup shares: the general kernel.  After init at 1024 x 1024 three
    passes are cut into regions of 768: no sharing, the closed instance.  And back."""
    scene, cam, opt, g = _scene("cornell")
    r = create_gpu_renderer(scene)
    small, plan_small = _render(scene, cam, opt, 16, (32, 32), r=r)
    big, plan_big = _render(scene, cam, opt, 3, (1024, 1024), r=r)
    again, plan_again = _render(scene, cam, opt, 16, (32, 32), r=r)
    r.close()
    assert plan_small[0] == F.BOUNCE_GENERAL and plan_small[1] & F.BOUNCE_SHARE
    assert plan_big[0] == F.BOUNCE_FIT_CLOSED and not plan_big[1] & F.BOUNCE_SHARE
    assert plan_again == plan_small and np.array_equal(again, small)
    assert np.array_equal(small, _render(scene, cam, opt, 16, (32, 32), fit=0)[0])
    assert np.array_equal(big, _render(scene, cam, opt, 3, (1024, 1024), fit=0)[0])


@pytest.mark.parametrize("name", ["glass", "motionblur"])
def test_a_scene_outside_every_mask_plans_what_it_did(name):
    """glass and motionblur do not run the fused kernel at all: the switch changes neither the kernels they launch nor their image"""
    scene, cam, opt, g = _scene(name)
    outs = []
    for fit in (-1, 0):
        r = create_gpu_renderer(scene, 0, abi.Tuning(bounce_fit=fit))
        r.enable_kernel_timing(True)
        r.init(opt.width, opt.height)
        out = r.render(cam, opt, passes=int(g["passes"]))
        outs.append((out, sorted(r.kernel_times())))
        r.close()
    assert outs[0][1] == outs[1][1] and "k_bounce" not in outs[0][1], outs[0][1]
    assert scene.bounce_features() & (F.BOUNCE_MESH_WALK | F.BOUNCE_MOTION | F.BOUNCE_TRANSMISSION)       # (outside both compiled sets)
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][0], g["accum"])

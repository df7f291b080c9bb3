"""View batches without a GPU: the batch cut tinsel_hip_plan_views states against the header's rules, the camera helpers against a numpy
statement of what they promise, and the yardstick of the GPU tests (tests/views_reference.py) for the reference alone."""
import ctypes as C
import math

import numpy as np
import pytest

import tinsel_amd
from tinsel_amd import abi
from tests import views_reference as vr


# ---------------------------------------------------------------------------
# tinsel_hip_plan_views

def _rule(limit, width, height, passes, views):
    """the header's rule, restated"""
    npix = width*height
    limit = min(limit, 2**32 - 2)
    per_view = npix*passes
    if per_view <= limit:
        vpb = min(views, limit//per_view)
        return vpb, passes, -(-views//vpb)
    ppb = min(passes, max(1, limit//npix))
    return 1, ppb, views*(-(-passes//ppb))


PLAN_CASES = {
    "everything_fits": (64 << 20, 128, 128, 4, 64, (64, 4, 1)),
    "several_views_and_a_remainder": (2*3*40*24, 40, 24, 3, 5, (2, 3, 3)),
    "one_view_cut_into_pass_batches": (2*40*24 + 17, 40, 24, 5, 3, (1, 2, 9)),
    "a_single_pass_larger_than_the_limit": (512, 40, 24, 3, 5, (1, 1, 15)),
    "one_view": (64 << 20, 256, 256, 16, 1, (1, 16, 1)),
    "one_view_cut": (3*256*256, 256, 256, 16, 1, (1, 3, 6)),
    "a_limit_beyond_32_bits": (1 << 40, 1024, 1024, 16, 4096, (255, 16, 17)),
}


@pytest.mark.parametrize("case", sorted(PLAN_CASES))
def test_plan_views_states_the_cut(case):
    limit, width, height, passes, views, want = PLAN_CASES[case]
    got = tinsel_amd.plan_views(limit, width, height, passes, views)
    assert got == want == _rule(limit, width, height, passes, views), (case, got)
    vpb, ppb, batches = got
    assert vpb >= 1 and ppb >= 1                                # at least one pass of one view per batch
    assert vpb*ppb*width*height < 2**32 - 1                     # no batch has 2^32 - 1 slots or more
    assert vpb == 1 or ppb == passes                            # several views per batch only with all their passes
    assert vpb*ppb*width*height <= max(limit, width*height)     # under the limit, but for a single pass larger than it


def test_plan_views_over_a_sweep_and_its_refusals():
    rng = np.random.RandomState(5)
    for _ in range(300):
        width, height = int(rng.randint(1, 300)), int(rng.randint(1, 300))
        passes, views = int(rng.randint(1, 40)), int(rng.randint(1, 4097))
        limit = int(2**rng.uniform(0, 34))
        assert tinsel_amd.plan_views(limit, width, height, passes, views) == _rule(limit, width, height, passes, views)
    L = tinsel_amd.load_library()
    out = (C.c_int*3)()
    for args in ((1 << 20, 0, 24, 1, 1), (1 << 20, 40, 24, 0, 1), (1 << 20, 40, 24, 1, 0), (1 << 20, 65536, 65536, 1, 1)):
        assert L.tinsel_hip_plan_views(*args, out) == -1 and L.tinsel_hip_last_error()
    assert L.tinsel_hip_plan_views(1 << 20, 40, 24, 1, 1, None) == -1
    assert abi.MAX_VIEWS == 4096 and (abi.VIEWS_ADD, abi.VIEWS_ACCUMULATE_SINGLY) == (1, 2)


# ---------------------------------------------------------------------------
# the camera helpers

def _camera():
    cam, _ = vr.frame("cornell")
    cam.shutter_start, cam.shutter_end = 0.25, 0.75
    return cam


@pytest.mark.parametrize("axis", [(0, 1, 0), (1, 2, -0.5)])
def test_orbit_cameras_turn_position_and_rotation_about_the_axis(axis):
    cam = _camera()
    center = np.array([0.1, 0.5, -0.2])
    n = np.asarray(axis, np.float64)/np.linalg.norm(axis)
    count = 7
    cams = tinsel_amd.orbit_cameras(cam, center, count, axis)
    assert len(cams) == count and bytes(cams[0]) == bytes(cam)              # k = 0: the camera itself, bit for bit
    p0 = np.array(tuple(cam.position), np.float64)
    r0, u0, f0 = vr.camera_axes(cam)
    radius = np.linalg.norm(np.cross(n, p0 - center))
    for k in range(count):
        c = cams[k]
        assert (c.fov, c.shutter_start, c.shutter_end) == (cam.fov, cam.shutter_start, cam.shutter_end)
        R = vr.quat_matrix(vr.quat_axis_angle(n, 2*math.pi*k/count))
        p = np.array(tuple(c.position), np.float64)
        # on the circle: the same distance from the axis, the same height along it, the angle 2*pi*k/count
        assert np.allclose(p, center + R @ (p0 - center), atol=1e-5)
        assert abs(np.linalg.norm(np.cross(n, p - center)) - radius) < 1e-5 and abs(np.dot(n, p - p0)) < 1e-5
        # the rotation is turned with it: the camera keeps looking at what it looked at
        r, u, f = vr.camera_axes(c)
        assert np.allclose(r, R @ r0, atol=1e-5) and np.allclose(u, R @ u0, atol=1e-5) and np.allclose(f, R @ f0, atol=1e-5)
        assert abs(np.linalg.norm(tuple(c.rotation)) - 1.0) < 1e-6
    assert len(tinsel_amd.orbit_cameras(cam, center, 1)) == 1
    with pytest.raises(ValueError):
        tinsel_amd.orbit_cameras(cam, center, 0)
    with pytest.raises(ValueError):
        tinsel_amd.orbit_cameras(cam, center, 3, (0, 0, 0))


def test_cube_cameras_look_along_the_six_axes():
    cams = tinsel_amd.cube_cameras((1.0, 2.0, 3.0), shutter=(0.1, 0.9))
    assert len(cams) == 6
    want_forward = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    want_up = [(0, 1, 0), (0, 1, 0), (0, 0, 1), (0, 0, -1), (0, 1, 0), (0, 1, 0)]       # the docstring's
    forwards = []
    for c, wf, wu in zip(cams, want_forward, want_up):
        assert tuple(c.position) == (1.0, 2.0, 3.0) and c.fov == np.float32(math.pi/2) and (c.shutter_start, c.shutter_end) == (np.float32(0.1), np.float32(0.9))
        r, u, f = vr.camera_axes(c)
        assert np.allclose(f, wf, atol=1e-6) and np.allclose(u, wu, atol=1e-6) and np.allclose(r, np.cross(f, u), atol=1e-6)
        forwards.append(f)
    # six orthogonal forward axes: every pair is opposite or at right angles
    g = np.array(forwards) @ np.array(forwards).T
    assert np.allclose(np.abs(g), np.eye(6) + np.eye(6)[[1, 0, 3, 2, 5, 4]], atol=1e-6)
    # the identity rotation is the -z face: the reference's camera looks along its local -z
    assert tuple(cams[5].rotation) == (0.0, 0.0, 0.0, 1.0)


def test_views_binds_and_refuses_without_a_renderer():
    L = tinsel_amd.load_library()
    cams = tinsel_amd.cube_cameras((0, 0, 0))
    _, opt = vr.frame("cornell")
    out = np.full((6, vr.H, vr.W, 4), 7.0, np.float32)
    assert L.tinsel_hip_render_views(None, cams, 6, C.byref(opt), 0, 1, 0, out.ctypes.data_as(C.c_void_p)) == -1
    assert b"null argument" in L.tinsel_hip_last_error() and (out == 7.0).all()
    assert L.tinsel_hip_render_views_device(None, cams, 6, C.byref(opt), 0, 1, 0, out.ctypes.data_as(C.c_void_p), None) == -1


# ---------------------------------------------------------------------------
# the yardstick for the reference alone

def test_the_yardstick_tells_cameras_apart():
    cam, opt = vr.frame("cornell")
    other = vr.turned(cam, yaw=0.2)
    a = vr.oracle_view("cornell", cam, opt, 0, 2)
    b = vr.oracle_view("cornell", other, opt, 0, 2)
    again = vr.oracle_view("cornell", abi.Camera.from_buffer_copy(bytes(cam)), opt, 0, 2)
    assert a.shape == (vr.H, vr.W, 4) and a.dtype == np.float32 and np.isfinite(a).all() and a[..., :3].any()
    assert np.array_equal(a, again)
    assert not np.array_equal(a, b) and np.array_equal(a[..., 3], b[..., 3])          # the raster positions are the seeds' alone
    # (and without the cache: a second run of the oracle gives the same bits)
    fresh = vr._render.__wrapped__("cornell", bytes(cam), bytes(opt), 0, 2)
    assert np.array_equal(a, fresh)

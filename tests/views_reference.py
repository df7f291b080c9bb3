"""The yardstick of the view-batch tests: plane v of tinsel_hip_render_views is the accumulator of cameras[v] alone -- the oracle's
render_seeded(h, camera, options, pass_begin, passes) per camera, through tests/oracle_api.py, the oracle chosen as the light-group tests
choose it -- and the few lines of numpy quaternion arithmetic the camera helpers are held to.  Renders are computed once per (pack, camera,
options, passes), shared and left unchanged."""
import functools
import os

import numpy as np

from tinsel_amd import abi
from tests import oracle_api as oa
from tests import light_groups_reference as lg

W, H = 40, 24           # three by two accumulate tiles, both edges ragged

oracle = lg.oracle
pack_bytes = functools.lru_cache(maxsize=None)(lg.pack_bytes)


def frame(name, width=W, height=H):
    """(camera, options) of the pack at the tests' frame size"""
    return lg.frame(pack_bytes(name), width, height)


@functools.lru_cache(maxsize=None)
def _render(name, cam_bytes, opt_bytes, pass_begin, passes):
    cam, opt = abi.Camera.from_buffer_copy(cam_bytes), abi.Options.from_buffer_copy(opt_bytes)
    O = oracle()
    h = O.load_pack(pack_bytes(name))
    try:
        out, _, _ = O.render_seeded(h, cam, opt, pass_begin, passes, threads=min(16, os.cpu_count() or 1))
    finally:
        O.free(h)
    out.setflags(write=False)
    return out


def oracle_view(name, cam, opt, pass_begin, passes):
    """the oracle's accumulator of one camera: float32 [H, W, 4], read-only"""
    return _render(name, bytes(cam), bytes(opt), int(pass_begin), int(passes))


def oracle_views(name, cameras, opt, pass_begin, passes):
    return np.stack([oracle_view(name, c, opt, pass_begin, passes) for c in cameras])


# --- quaternions (x, y, z, w), float64

def quat_axis_angle(axis, angle):
    n = np.asarray(axis, np.float64)
    n = n/np.linalg.norm(n)
    return np.concatenate([n*np.sin(0.5*angle), [np.cos(0.5*angle)]])


def quat_matrix(q):
    """the rotation matrix of a unit quaternion: its columns are the images of e_x, e_y, e_z"""
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2*(y*y + z*z), 2*(x*y - z*w), 2*(x*z + y*w)],
                     [2*(x*y + z*w), 1 - 2*(x*x + z*z), 2*(y*z - x*w)],
                     [2*(x*z - y*w), 2*(y*z + x*w), 1 - 2*(x*x + y*y)]])


def camera_axes(cam):
    """(right, up, forward) of a camera in world space: the reference's camera looks along its local -z with +y up"""
    m = quat_matrix(tuple(cam.rotation))
    return m[:, 0], m[:, 1], -m[:, 2]


def turned(cam, yaw=0.0, pitch=0.0, shift=(0.0, 0.0, 0.0), shutter=None):
    """a copy of the camera turned about the world's y (then its own x) where it stands, moved by `shift`"""
    out = abi.Camera.from_buffer_copy(bytes(cam))
    q0 = np.array(tuple(cam.rotation), np.float64)
    m = quat_matrix(quat_axis_angle((0, 1, 0), yaw)) @ quat_matrix(q0) @ quat_matrix(quat_axis_angle((1, 0, 0), pitch))
    # matrix -> quaternion (w is largest for the small turns used here, and positive)
    w = 0.5*np.sqrt(max(0.0, 1.0 + m[0, 0] + m[1, 1] + m[2, 2]))
    if w > 1e-3:
        q = np.array([(m[2, 1] - m[1, 2])/(4*w), (m[0, 2] - m[2, 0])/(4*w), (m[1, 0] - m[0, 1])/(4*w), w])
    else:
        x = 0.5*np.sqrt(max(0.0, 1.0 + m[0, 0] - m[1, 1] - m[2, 2]))
        y = 0.5*np.sqrt(max(0.0, 1.0 - m[0, 0] + m[1, 1] - m[2, 2]))
        z = 0.5*np.sqrt(max(0.0, 1.0 - m[0, 0] - m[1, 1] + m[2, 2]))
        k = int(np.argmax([x, y, z]))
        if k == 0:
            q = np.array([x, (m[0, 1] + m[1, 0])/(4*x), (m[0, 2] + m[2, 0])/(4*x), (m[2, 1] - m[1, 2])/(4*x)])
        elif k == 1:
            q = np.array([(m[0, 1] + m[1, 0])/(4*y), y, (m[1, 2] + m[2, 1])/(4*y), (m[0, 2] - m[2, 0])/(4*y)])
        else:
            q = np.array([(m[0, 2] + m[2, 0])/(4*z), (m[1, 2] + m[2, 1])/(4*z), z, (m[1, 0] - m[0, 1])/(4*z)])
    q = q/np.linalg.norm(q)
    out.rotation = abi.Vec4(*(float(v) for v in q))
    p = np.array(tuple(cam.position), np.float64) + np.asarray(shift, np.float64)
    out.position = abi.Vec3(*(float(v) for v in p))
    if shutter is not None:
        out.shutter_start, out.shutter_end = float(shutter[0]), float(shutter[1])
    return out


def five_cameras(name, shutters=None):
    """The tests' five views of a pack: its own camera, two turned left and right, one pitched and moved a little, and one turned to look
    straight up (on veach: at the sky alone).  shutters: five (start, end) pairs."""
    cam, _ = frame(name)
    cams = [cam, turned(cam, yaw=0.2), turned(cam, yaw=-0.25, shift=(0.1, 0.0, 0.0)), turned(cam, pitch=-0.15, shift=(0.0, 0.1, 0.05)),
            turned(cam, pitch=0.5*np.pi)]
    if shutters is not None:
        for c, (a, b) in zip(cams, shutters):
            c.shutter_start, c.shutter_end = float(a), float(b)
    return cams

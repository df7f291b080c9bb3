"""The yardstick of the light-group tests: plane g of tinsel_hip_render_light_groups is the render of the MASKED scene -- the same pack with
the emission of every primitive outside the group, and the sky unless the group holds it, set to zero -- so all a test needs of its own is
the byte edit that makes such a pack, and the rounding bound that the sums of planes are held to.  The renders themselves come from the
oracle the parity tests use (tests/oracle_api.py)."""
import ctypes as C
import functools
import os

import numpy as np

from tinsel_amd import abi
from tests import oracle_api as oa

PRIM_BYTES = C.sizeof(abi.Primitive)                                            # 272
EMISSION_AT = abi.Primitive.material.offset + abi.Material.emission.offset      # 136: 12 bytes
SKY_AT = abi.PackHeader.sky_horizon.offset                                      # 96: horizon and zenith, 24 bytes
assert (PRIM_BYTES, EMISSION_AT, SKY_AT, abi.PackHeader.sky_zenith.offset) == (272, 136, 96, 108)


def header(blob):
    return abi.PackHeader.from_buffer_copy(bytes(blob[:C.sizeof(abi.PackHeader)]))


def emission(blob, i):
    at = header(blob).off_primitives + PRIM_BYTES*i + EMISSION_AT
    return np.frombuffer(bytes(blob[at:at + 12]), np.float32)


def emitters(blob):
    """the primitives whose emission is not all zero, in index order"""
    return [i for i in range(header(blob).num_primitives) if emission(blob, i).any()]


def has_sky(blob):
    return bool(np.frombuffer(bytes(blob[SKY_AT:SKY_AT + 24]), np.float32).any())


def with_emission(blob, i, rgb):
    """the pack with primitive i's emission set (light_samples stays what it is: a wall that emits is found by BSDF rays only)"""
    out = bytearray(blob)
    at = header(blob).off_primitives + PRIM_BYTES*i + EMISSION_AT
    out[at:at + 12] = np.asarray(rgb, np.float32).tobytes()
    return bytes(out)


def masked_pack(blob, keep, keep_sky):
    """The pack with emission = 0 on every primitive not in `keep` and, unless keep_sky, sky horizon = zenith = 0: 12 bytes at
    off_primitives + 272*i + 136 per primitive, 24 bytes at header offset 96.  A probe is not touched.  Nothing else of a primitive changes:
    its area, its light_samples and with them every sampling decision stay."""
    out = bytearray(blob)
    h = header(blob)
    keep = set(int(i) for i in keep)
    for i in range(h.num_primitives):
        if i not in keep:
            at = h.off_primitives + PRIM_BYTES*i + EMISSION_AT
            out[at:at + 12] = bytes(12)
    if not keep_sky:
        out[SKY_AT:SKY_AT + 24] = bytes(24)
    return bytes(out)


def rounding_c(max_depth, passes):
    """c of |sum - beauty| <= c*(sum + beauty): a path sums at most 2*max_depth + 1 non-negative terms and a pixel `passes` samples (times
    the filter's footprint, which the weight channel normalises alike on both sides), all non-negative, so each rounding is at most 2^-24 of
    the final value; the factor 2 and the + 4 are slack."""
    return 2.0*(2*int(max_depth) + int(passes) + 4)*2.0**-24


@functools.lru_cache(maxsize=None)
def oracle():
    """the reference's own PathTrace where oracle/_ref travelled here, else its plain-C restatement (what __graft_entry__.smoke uses)"""
    return oa.RefOracle() if oa.have_ref() else oa.PortOracle()


def pack_bytes(name):
    with open(os.path.join(oa.GOLDEN, name + ".pack"), "rb") as fh:
        return fh.read()


def frame(blob, width, height, clamp=None):
    """(camera, options) of the pack at another frame size (and clamp)"""
    h = header(blob)
    cam, opt = abi.Camera.from_buffer_copy(bytes(h.camera)), abi.Options.from_buffer_copy(bytes(h.options))
    opt.width, opt.height = width, height
    if clamp is not None:
        opt.clamp = clamp
    return cam, opt


def oracle_render(blob, cam, opt, pass_begin, passes):
    O = oracle()
    h = O.load_pack(blob)
    try:
        out, _, _ = O.render_seeded(h, cam, opt, pass_begin, passes, threads=min(16, os.cpu_count() or 1))
    finally:
        O.free(h)
    out.setflags(write=False)
    return out

"""Light groups (tinsel_hip_render_light_groups / _device, kernel k_shade_groups): the beauty split per emitter group in one trace.

The yardstick is not under test: plane g is, bit for bit in all four channels, the oracle's render of the MASKED pack -- the emission of
every primitive outside the group, and the sky unless the group holds it, zeroed (tests/light_groups_reference.py; the oracle is the one the
parity tests use).  Every case renders 48 x 32 pixels, 4 passes from pass 0, with the pack's own options unless it says otherwise; oracle
renders are computed once, shared and left unchanged.

Figures (MI355X): the bit-for-bit cases have none; the bounded ones print their worst pixel as a fraction of the bound before they assert."""
import ctypes as C
import functools

import numpy as np
import pytest

import tinsel_amd
from tinsel_amd import abi
from tests import light_groups_reference as lg

pytestmark = pytest.mark.gpu

W, H, PASSES = 48, 32, 4
FLT_MAX = float(np.finfo(np.float32).max)
PIPELINES = {"auto": abi.PIPELINE_AUTO, "wavefront": abi.PIPELINE_WAVEFRONT, "mega": abi.PIPELINE_MEGAKERNEL, "split": abi.PIPELINE_WAVEFRONT_SPLIT,
             "paired": abi.PIPELINE_WAVEFRONT_PAIRED}


@functools.lru_cache(maxsize=None)
def _blob(name):
    if name == "cornell_wall":          # a wall (light_samples == 0) emits: found by BSDF rays only
        blob = lg.with_emission(lg.pack_bytes("cornell"), 0, (0.5, 0.375, 0.25))
        assert C.cast(tinsel_amd.Scene(blob).desc.primitives, C.POINTER(abi.Primitive))[0].light_samples == 0
        return blob
    return lg.pack_bytes(name)


@functools.lru_cache(maxsize=None)
def _masked(name, keep, sky, width=W, height=H, pass_begin=0, clamp=None):
    """the oracle's render of the pack masked to the primitives `keep` (and the sky): the yardstick of one plane"""
    blob = _blob(name)
    cam, opt = lg.frame(blob, width, height, clamp)
    out = lg.oracle_render(lg.masked_pack(blob, keep, sky), cam, opt, pass_begin, PASSES)
    assert np.isfinite(out).all(), (name, keep, sky)
    return out


def _open(name, width=W, height=H, clamp=None):
    blob = _blob(name)
    scene = tinsel_amd.Scene(blob)
    r = tinsel_amd.create_gpu_renderer(scene)
    r.init(width, height)
    cam, opt = lg.frame(blob, width, height, clamp)
    return scene, r, cam, opt


def _table(name, groups):
    t = np.full(lg.header(_blob(name)).num_primitives, -1, np.int32)
    for g, prims in enumerate(groups):
        t[list(prims)] = g
    return t


def _same(got, want, what):
    assert got.dtype == np.float32 and got.shape == want.shape, what
    bad = (got != want).any(axis=-1)
    first = np.unravel_index(np.argmax(bad), bad.shape)
    assert np.array_equal(got, want), "%s: %d of %d pixels differ (first: %s, %s against %s)" % (what, int(bad.sum()), bad.size, first, got[first], want[first])


def _one_group(name):
    """(scene, groups, where the sky goes): every emitter in group 0, and the sky with them where the scene has one"""
    return name, [tuple(lg.emitters(_blob(name)))], "group0" if lg.has_sky(_blob(name)) else "none"


# ---------------------------------------------------------------------------
# 1: exact, per group, against the oracle's masked render

VEACH_GROUPS = [(5,), (6,), (7,), (8,)]
# scene, the primitives of each group, the sky ("none": the scene has none; "own": the group after the lights; "group0": with group 0), frame
CASES = {
    "veach": ("veach", VEACH_GROUPS, "none", {}),                                   # one group per light
    "features": ("features", [(2,), (3,)], "own", {}),                              # lights with 2 and 3 samples, the sky on
    "many_spheres": ("many_spheres", [(1,), (2,)], "own", {}),                      # 203 primitives: the scene-level walk
    "glass": _one_group("glass") + ({},),                                           # media, depth 8
    "motionblur": _one_group("motionblur") + ({},),                                 # a moving mesh light with 10 samples, meshes in HBM
    "cornell_wall": ("cornell_wall", [(5,), (0,)], "none", {}),                     # an emitter that is no light
    "veach_50x34": ("veach", VEACH_GROUPS, "none", {"width": 50, "height": 34}),    # ragged tiles
    "veach_pass3": ("veach", VEACH_GROUPS, "none", {"pass_begin": 3}),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_plane_is_the_oracles_masked_render(case):
    name, groups, sky, how = CASES[case]
    width, height, pass_begin = how.get("width", W), how.get("height", H), how.get("pass_begin", 0)
    assert set(sum(groups, ())) == set(lg.emitters(_blob(name))) and (sky != "none") == lg.has_sky(_blob(name))
    env = {"none": -1, "own": len(groups), "group0": 0}[sky]
    scene, r, cam, opt = _open(name, width, height)
    try:
        planes = r.light_groups(cam, opt, pass_begin, PASSES, _table(name, groups), env)
    finally:
        r.close()
    assert planes.shape == (len(groups) + (1 if sky == "own" else 0), height, width, 4)
    for g, prims in enumerate(groups):
        want = _masked(name, prims, sky == "group0" and g == 0, width, height, pass_begin)
        _same(planes[g], want, "%s, group %d = primitives %s" % (case, g, prims))
        assert want[..., :3].any(), (case, g)
    if sky == "own":
        _same(planes[env], _masked(name, (), True, width, height, pass_begin), "%s, the environment" % case)


# ---------------------------------------------------------------------------
# 2: grouping

def test_lights_share_a_group():
    scene, r, cam, opt = _open("veach")
    try:
        planes = r.light_groups(cam, opt, 0, PASSES, _table("veach", [(5, 7), (6, 8)]))
    finally:
        r.close()
    assert planes.shape[0] == 2
    _same(planes[0], _masked("veach", (5, 7), False), "veach {5, 7}")
    _same(planes[1], _masked("veach", (6, 8), False), "veach {6, 8}")


def test_a_primitive_in_no_group_reaches_no_plane():
    scene, r, cam, opt = _open("veach")
    try:
        planes = r.light_groups(cam, opt, 0, PASSES, _table("veach", [(5, 7, 8)]))          # 6: -1
    finally:
        r.close()
    assert planes.shape[0] == 1
    _same(planes[0], _masked("veach", (5, 7, 8), False), "veach without 6")
    assert not np.array_equal(planes[0], _masked("veach", (5, 6, 7, 8), False))


@pytest.mark.parametrize("name", ["features", "veach"])
def test_everything_in_one_group_is_the_render(name):
    scene, r, cam, opt = _open(name)
    try:
        _, groups, sky = _one_group(name)
        planes = r.light_groups(cam, opt, 0, PASSES, _table(name, groups), 0 if sky == "group0" else -1)
        beauty = r.render(cam, opt, passes=PASSES)
    finally:
        r.close()
    assert planes.shape[0] == 1
    _same(planes[0], beauty, "%s, G = 1 against tinsel_hip_render" % name)


# ---------------------------------------------------------------------------
# 3: a probe scene

def test_the_probe_lands_in_the_environment_plane_only():
    """The environment plane is the oracle's render with every emission zeroed, exactly, under the pack's own options (clamp 8).
    A light's plane is held to |(M - E) - plane| <= c*(M + E), M the oracle's render masked to the group with the probe kept.  That bound
    is a rounding bound: it presumes that M, E and the plane are sums of the same terms, which ClampLength undoes (it applies to each
    render's whole path).  This scene has 204 of 6144 paths longer than its clamp of 8, and there the REFERENCE ALONE misses the
    corresponding bound -- M2 + M3 - E - beauty against c*(M2 + M3 + E + beauty) -- by a factor of 2392, while with clamp = FLT_MAX it stays
    within 0.041 of it.  So the bounded half runs with clamp = FLT_MAX, the environment plane is held exactly under both clamps, and the
    planes under the pack's own clamp are held to their definition exactly where it can be evaluated: the planes of a probe-free scene
    (case 1)."""
    name = "features_probe"
    assert tinsel_amd.Scene(_blob(name)).desc.probe_valid and lg.emitters(_blob(name)) == [2, 3]
    table = _table(name, [(2,), (3,)])
    scene, r, cam, opt = _open(name)
    try:
        assert opt.clamp == 8.0
        own = r.light_groups(cam, opt, 0, PASSES, table, 2)
        free = opt.copy()
        free.clamp = FLT_MAX
        planes = r.light_groups(cam, free, 0, PASSES, table, 2)
    finally:
        r.close()
    # every emission zeroed; the probe is not part of the mask
    _same(own[2], _masked(name, (), True), "features_probe, the environment, the pack's clamp")
    E = _masked(name, (), True, clamp=FLT_MAX)
    _same(planes[2], E, "features_probe, the environment, no clamp")
    c = lg.rounding_c(opt.max_depth, PASSES)
    for g, prim in enumerate((2, 3)):
        M = _masked(name, (prim,), True, clamp=FLT_MAX)         # masked to the group, the probe kept
        assert np.array_equal(planes[g][..., 3], M[..., 3]) and np.array_equal(own[g][..., 3], M[..., 3])
        m, e, p = (a[..., :3].astype(np.float64) for a in (M, E, planes[g]))
        bound = c*(m + e)
        err = np.abs((m - e) - p)
        worst = float((err/np.where(bound > 0, bound, 1.0)).max())
        print("features_probe group {%d}: worst |(M - E) - plane| = %.4f of c*(M + E), c = %.3e" % (prim, worst, c))
        assert (err <= bound).all(), worst
        assert p.any() and np.isfinite(own[g]).all() and own[g][..., :3].any()


# ---------------------------------------------------------------------------
# 4: additivity without a clamp

@pytest.mark.parametrize("name", ["veach", "features"])
def test_the_planes_add_up_to_the_beauty_without_a_clamp(name):
    groups = [(i,) for i in lg.emitters(_blob(name))]
    sky = lg.has_sky(_blob(name))
    scene, r, cam, opt = _open(name, clamp=FLT_MAX)
    try:
        planes = r.light_groups(cam, opt, 0, PASSES, _table(name, groups), len(groups) if sky else -1)
        beauty = r.render(cam, opt, passes=PASSES)
    finally:
        r.close()
    for g in range(planes.shape[0]):
        assert np.array_equal(planes[g][..., 3].view(np.uint32), beauty[..., 3].view(np.uint32)), (name, g)
    total = planes[..., :3].astype(np.float64).sum(axis=0)
    b = beauty[..., :3].astype(np.float64)
    bound = lg.rounding_c(opt.max_depth, PASSES)*(total + b)
    worst = float((np.abs(total - b)/np.where(bound > 0, bound, 1.0)).max())
    print("%s: %d planes, worst |sum - beauty| = %.4f of the bound" % (name, planes.shape[0], worst))
    assert (np.abs(total - b) <= bound).all(), worst
    # ... and with the scene's own clamp each plane is still its masked render (case 1), which is why the sum then differs
    assert np.isfinite(planes).all()


# ---------------------------------------------------------------------------
# 5: independence

@functools.lru_cache(maxsize=None)
def _veach_planes():
    scene, r, cam, opt = _open("veach")
    try:
        out = r.light_groups(cam, opt, 0, PASSES, _table("veach", VEACH_GROUPS))
    finally:
        r.close()
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("pipeline", sorted(PIPELINES))
def test_the_pipeline_setting_does_not_show(pipeline):
    scene, r, cam, opt = _open("veach")
    try:
        r.set_pipeline(PIPELINES[pipeline])
        planes = r.light_groups(cam, opt, 0, PASSES, _table("veach", VEACH_GROUPS))
    finally:
        r.close()
    _same(planes, _veach_planes(), "veach under set_pipeline(%s)" % pipeline)


def test_the_batch_cut_does_not_show():
    scene, r, cam, opt = _open("veach")
    try:
        r.enable_kernel_timing(True)
        r.set_batch_paths(W*H)                                                              # one pass per batch: four batches
        planes = r.light_groups(cam, opt, 0, PASSES, _table("veach", VEACH_GROUPS))
        times = r.kernel_times()
    finally:
        r.close()
    _same(planes, _veach_planes(), "veach, one pass per batch")
    # four batches: k_generate once each, k_accumulate once per plane and batch, the twin under k_shade's name once per bounce and batch
    assert times["k_generate"][0] == PASSES and times["k_accumulate"][0] == PASSES*len(VEACH_GROUPS)
    assert times["k_shade"][0] == PASSES*opt.max_depth


def test_the_device_entry_on_a_callers_stream():
    import torch
    scene, r, cam, opt = _open("veach")
    try:
        out = torch.full((len(VEACH_GROUPS), H, W, 4), 7.0, dtype=torch.float32, device="cuda:0")
        s = torch.cuda.Stream(device=0)
        s.wait_stream(torch.cuda.current_stream(0))
        with torch.cuda.stream(s):
            got = r.light_groups(cam, opt, 0, PASSES, _table("veach", VEACH_GROUPS), out=out)
        s.synchronize()
        assert got is out
        planes = out.cpu().numpy()
        # a render on the default stream afterwards finds the path buffers in order (the fence)
        beauty = r.render(cam, opt, passes=PASSES)
    finally:
        r.close()
    _same(planes, _veach_planes(), "veach, device entry")
    scene2, r2, cam2, opt2 = _open("veach")
    try:
        _same(beauty, r2.render(cam2, opt2, passes=PASSES), "the render behind the device entry")
    finally:
        r2.close()


@pytest.mark.parametrize("name", ["veach", "many_spheres"])
def test_a_call_between_two_renders_leaves_no_trace(name):
    groups = [(i,) for i in lg.emitters(_blob(name))]
    env = len(groups) if lg.has_sky(_blob(name)) else -1
    scene, r, cam, opt = _open(name)
    try:
        r.render(cam, opt, passes=2)
        before, index = r.stats(), r.get_pass_index()
        planes = r.light_groups(cam, opt, 0, PASSES, _table(name, groups), env)
        assert r.get_pass_index() == index == 2 and r.stats() == before
        split = r.render(cam, opt, passes=2)
    finally:
        r.close()
    scene, r, cam, opt = _open(name)
    try:
        whole = r.render(cam, opt, passes=4)
    finally:
        r.close()
    _same(split, whole, "%s: 2 passes, a light-groups call, 2 passes" % name)
    _same(planes[0], _masked(name, groups[0], False), "%s: the call between the renders" % name)


# ---------------------------------------------------------------------------
# 6: refusals

def test_refusals_leave_out_untouched():
    scene, r, cam, opt = _open("veach")
    L = tinsel_amd.load_library()
    try:
        out = np.full((2, H, W, 4), 5.0, np.float32)
        good = _table("veach", [(5, 7), (6, 8)])

        def refused(cause, table=good, env=-1, o=opt, passes=PASSES, groups=2, target=out):
            tp = table.ctypes.data_as(C.c_void_p) if table is not None else None
            op = target.ctypes.data_as(C.c_void_p) if target is not None else None
            rc = L.tinsel_hip_render_light_groups(r._h, C.byref(cam), C.byref(o), 0, passes, groups, tp, env, op)
            msg = L.tinsel_hip_last_error()
            assert rc == -1 and msg.startswith(b"render_light_groups:") and cause in msg, (cause, rc, msg)
            assert (out == 5.0).all(), cause

        refused(b"null", table=None)
        refused(b"null", target=None)
        refused(b"passes", passes=0)
        refused(b"num_groups", groups=0)
        refused(b"num_groups", groups=9)
        refused(b"env_group", env=2)
        refused(b"env_group", env=-2)
        for bad in (2, -2):
            t = good.copy()
            t[3] = bad
            refused(b"group_of_primitive[3]", table=t)
        other = opt.copy()
        other.width = W + 1
        refused(b"tinsel_hip_init", o=other)
        normals = opt.copy()
        normals.mode = abi.MODE_NORMALS
        refused(b"mode", o=normals)
        r.set_arithmetic(abi.ARITH_FAST)
        refused(b"TINSEL_ARITH_FAST")
        r.set_arithmetic(abi.ARITH_EXACT)
        r.set_shard(0, 2, 16)
        refused(b"sharded")
        r.set_shard(0, 1, 16)
        # the device entry: a misaligned array
        import torch
        dev = torch.full((2*H*W*4 + 4,), 5.0, dtype=torch.float32, device="cuda:0")
        rc = L.tinsel_hip_render_light_groups_device(r._h, C.byref(cam), C.byref(opt), 0, PASSES, 2, good.ctypes.data_as(C.c_void_p), -1,
                                                     dev.data_ptr() + 4, None)
        assert rc == -1 and b"16-byte aligned" in L.tinsel_hip_last_error()
        torch.cuda.synchronize()
        assert bool((dev == 5.0).all())
        # ... and after all of that the call still works; max_depth < 1 gives all-zero planes
        planes = r.light_groups(cam, opt, 0, PASSES, good)
        _same(planes[0], _masked("veach", (5, 7), False), "veach {5, 7} after the refusals")
        flat = opt.copy()
        flat.max_depth = 0
        assert not r.light_groups(cam, flat, 0, PASSES, good, out=out).any()
        # a moved primitive without a rebuild
        out[:] = 5.0
        prims = C.cast(scene.desc.primitives, C.POINTER(abi.Primitive))
        r.set_primitive_transform(0, abi.Transform.from_buffer_copy(bytes(prims[0].start_transform)))
        refused(b"tinsel_hip_rebuild_scene")
    finally:
        r.close()

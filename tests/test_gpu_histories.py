"""A long-lived renderer is held to a fresh one after any history of calls (DESIGN.md "What a renderer's history may not change").

tests/renderer_model.py draws seeded schedules of API calls and keeps the LOGICAL state they lead to; tests/test_renderer_model.py checks on
the CPU what the committed schedules cover.  Here one live renderer runs a schedule in order.  At every observation a fresh renderer --
default tuning, pipeline AUTO, no look-ahead, nothing reserved -- is brought to the model's state by the shortest route (renderer_model.replay),
makes the same observation once and is closed, and the two results must agree bit for bit (compared as uint32 words: NaN payloads included).
After every op that must change nothing the pass index is checked at once, and at the end the accumulator; around a light-group, view-batch,
sample-map or depth-plane call the live renderer's statistics must stay as they were.  The bake mode (set_bake) is a live-only setting like
the pipeline: the fresh renderers never get it, and the module's baked instances share one cache directory.  A schedule on a scene with a golden
file ends on that file's own frame: the live renderer, after its whole history, is held to the reference's output, so that the fresh renderer
cannot be wrong in the same way unseen.

A mismatch names the seed, the step, the op, how many words differ and the first of them, and prints the schedule up to that step as a literal:
    from tests.test_gpu_histories import run_schedule; run_schedule([...])
replays it.  There is no shrinking loop."""
import contextlib
import os
import time

import numpy as np
import pytest

from tests import renderer_model as rm

pytestmark = pytest.mark.gpu

SECONDS_PER_SCHEDULE = 120          # a schedule takes a few seconds; one that takes this long ends itself at its next step


@pytest.fixture(scope="module", autouse=True)
def bake_cache(tmp_path_factory):
    """the baked instances the set_bake ops compile share one cache directory of the module's own: a scene level is compiled once"""
    from tinsel_amd import build as hb
    was = os.environ.get(hb.BAKE_CACHE_ENV)
    os.environ[hb.BAKE_CACHE_ENV] = str(tmp_path_factory.mktemp("bake_cache"))
    yield os.environ[hb.BAKE_CACHE_ENV]
    if was is None:
        del os.environ[hb.BAKE_CACHE_ENV]
    else:
        os.environ[hb.BAKE_CACHE_ENV] = was


class Mismatch(AssertionError):
    def __init__(self, step, op, what, ops, seed=None):
        self.step, self.op = step, op
        super().__init__("seed %s, step %d, op %r: %s\nthe schedule up to that step:\n%r" % (seed, step, op, what, list(ops[:step + 1])))


def _words(a):
    a = np.ascontiguousarray(a)
    if a.dtype.fields:                                  # a record array: its named 32-bit fields, not the reserved words
        return np.stack([a[n].view(np.uint32).reshape(-1) for n in a.dtype.names if a.dtype[n].shape == ()], axis=-1)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a.astype(np.int64)


def _differ(got, want):
    """None, or what differs between two observations (lists of arrays)"""
    if len(got) != len(want):
        return "%d results against %d" % (len(got), len(want))
    for k, (a, b) in enumerate(zip(got, want)):
        a, b = _words(a), _words(b)
        if a.shape != b.shape:
            return "result %d: shape %s, the fresh renderer's %s" % (k, a.shape, b.shape)
        bad = a != b
        if bad.any():
            first = tuple(int(i) for i in np.argwhere(bad)[0])
            return "result %d: %d of %d words differ, the first at %s: 0x%08x, the fresh renderer's 0x%08x" % (
                k, int(bad.sum()), bad.size, first, int(a[first]), int(b[first]))
    return None


# -- scenes, cameras, inputs: made once and left unchanged ----------------------------------------------------------------------------------------

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _scene(key):
    import tinsel_amd
    return _cached(("scene", key), lambda: tinsel_amd.Scene(rm.pack_bytes(key)))


def _frame(family):
    """(camera, options) a family renders with: the golden file's where there is one, else the pack's own"""
    from tinsel_amd import abi

    def make():
        g = rm.FAMILIES[family]["golden"]
        if g:
            z = np.load(os.path.join(rm.GOLDEN, g + ".golden.npz"))
            return abi.Camera.from_buffer_copy(z["camera"].tobytes()), abi.Options.from_buffer_copy(z["options"].tobytes())
        s = _scene(("pack", rm.FAMILIES[family]["pack"]))
        return s.camera, s.options
    return _cached(("frame", family), make)


def _options(family, size, depth=None, mode="pathtrace"):
    from tinsel_amd import abi
    o = _frame(family)[1].copy()
    o.width, o.height = size
    o.mode = abi.MODE_PATHTRACE if mode == "pathtrace" else abi.MODE_NORMALS
    if depth is not None:
        o.max_depth = depth
    return o


def _inputs(family):
    """rays, path starts and gather points about the camera: 4096 rays, 2048 path starts, 256 points x 8 samples"""
    from tinsel_amd import abi, gather_points, rng_state

    def make():
        cam = _frame(family)[0]
        rng = np.random.default_rng(20261020)
        d = rng.normal(size=(rm.N_RAYS, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        rays = np.zeros((rm.N_RAYS, 8), np.float32)
        rays[:, 0:3] = np.array([cam.position.x, cam.position.y, cam.position.z]) + rng.uniform(-0.05, 0.05, (rm.N_RAYS, 3))
        rays[:, 3] = rng.uniform(0.0, 1.0, rm.N_RAYS)
        rays[:, 4:7] = d
        rays[:, 7] = rng.choice([1e30, 3.0, 0.5], rm.N_RAYS)
        starts = np.zeros(rm.N_STARTS, abi.PATH_START_DTYPE)
        for k, n in enumerate(("ox", "oy", "oz", "time", "dx", "dy", "dz")):
            starts[n] = rays[:rm.N_STARTS, k]
        starts["rng1"], starts["rng2"] = rng_state(np.arange(rm.N_STARTS, dtype=np.uint32)*np.uint32(2654435761), 3)
        at = rays[:rm.N_POINTS, 0:3] + 0.5*rays[:rm.N_POINTS, 4:7]
        points = gather_points(at, -rays[:rm.N_POINTS, 4:7], rm.N_SAMPLES, time=rays[:rm.N_POINTS, 3], base_seed=77)
        return {"rays": rays, "starts": starts, "points": points}
    return _cached(("inputs", family), make)


def _device(family, name):
    import torch

    def make():
        a = _inputs(family)[name]
        words = a.view(np.float32).reshape(a.shape[0], -1) if a.dtype.fields else a
        return torch.from_numpy(np.ascontiguousarray(words)).cuda()
    return _cached(("device", family, name), make)


def _image(seed, size, weight=True):
    """an accumulator-form image [H, W, 4]: what write_accum, present_image and denoise on caller images are given"""
    def make():
        rng = np.random.default_rng(1000 + seed)
        a = rng.uniform(0.0, 4.0, (size[1], size[0], 4)).astype(np.float32)
        a[..., 3] = rng.uniform(0.5, 4.0, (size[1], size[0])).astype(np.float32) if weight else 1.0
        return a
    return _cached(("image", seed, tuple(size), weight), make)


def _orbit(family, count):
    """`count` cameras on a turntable about the point one unit in front of the family's camera (it looks along its local -z)"""
    from tinsel_amd import orbit_cameras

    def make():
        cam = _frame(family)[0]
        u, w = np.array(tuple(cam.rotation)[:3], np.float64), float(tuple(cam.rotation)[3])
        ahead = np.array([0.0, 0.0, -1.0])
        ahead = ahead + 2.0*np.cross(u, np.cross(u, ahead) + w*ahead)
        return orbit_cameras(cam, np.array(tuple(cam.position), np.float64) + ahead, count)
    return _cached(("orbit", family, count), make)


def _sample_map(name, size):
    """a uint16 pass count per pixel [H, W]: 2 everywhere, 0 .. 3 at random, a crop across column 16 and row 16, or 0 everywhere"""
    from tinsel_amd import crop_sample_map

    def make():
        W, H = size
        if name == "uniform":
            return np.full((H, W), 2, np.uint16)
        if name == "random":
            return np.random.default_rng(3000 + 100*W + H).integers(0, 4, (H, W)).astype(np.uint16)
        if name == "crop":
            return crop_sample_map(W, H, 10, 9, 23, 21, 3)
        assert name == "zeros", name
        return np.zeros((H, W), np.uint16)
    return _cached(("sample map", name, tuple(size)), make)


def _plane_count(r, feature, p):
    if feature == "light_groups":
        return rm.group_table(p["table"], r.num_primitives)[2]
    return {"views": p.get("count"), "sample_map": 1, "depth_planes": len(p.get("depths", ()))}[feature]


def planes_out(r, feature, p, state, device, fill=None):
    """The caller's `out` of a plane call: a numpy array (host entry) or a torch tensor (device entry, uploaded on torch's current stream)
    of zeros, with add one _image per plane from the op's seed (the same for every renderer), or full of `fill`."""
    import torch
    n, size = _plane_count(r, feature, p), state.size
    shape = (size[1], size[0], 4) if feature == "sample_map" else (n, size[1], size[0], 4)
    if fill is not None:
        out = np.full(shape, fill, np.float32)
    elif p.get("add"):
        out = np.stack([_image(p["seed"] + 10*k, size) for k in range(n)]).reshape(shape)
    else:
        out = np.zeros(shape, np.float32)
    return torch.from_numpy(out).cuda() if device else out


def plane_call(r, feature, p, state, device, out=None):
    """One call of a plane feature -- light groups, views, a sample map, depth planes -- on renderer `r`, through the host or the device
    entry (on torch's current stream): returns `out`"""
    fam, size = state.family, state.size
    cam, opt = _frame(fam)[0], _options(fam, size)
    if out is None:
        out = planes_out(r, feature, p, state, device)
    if feature == "light_groups":
        table, env, _ = rm.group_table(p["table"], r.num_primitives)
        return r.light_groups(cam, opt, p["pass_begin"], p["passes"], table, env, out=out)
    if feature == "views":
        return r.views(_orbit(fam, p["count"]), opt, p["pass_begin"], p["passes"], out=out, add=p["add"], singly=p["singly"])
    if feature == "sample_map":
        return r.sample_map(cam, opt, _sample_map(p["map"], size), p["pass_begin"], out=out, add=p["add"])
    return r.depth_planes(cam, opt, p["pass_begin"], p["passes"], p["depths"], out=out, add=p["add"], singly=p["singly"])


@contextlib.contextmanager
def _stream(side):
    """device entries run on torch's current stream: a non-default one where the schedule says so.  The result is read inside, in that
    stream's order; nothing is synchronised on leaving."""
    import torch
    if side:
        with torch.cuda.stream(_cached("side stream", torch.cuda.Stream)):
            yield
    else:
        yield


# -- one renderer, one op -------------------------------------------------------------------------------------------------------------------------

PIPELINE = {"auto": "PIPELINE_AUTO", "wavefront": "PIPELINE_WAVEFRONT", "split": "PIPELINE_WAVEFRONT_SPLIT",
            "paired": "PIPELINE_WAVEFRONT_PAIRED", "megakernel": "PIPELINE_MEGAKERNEL"}


def observe(r, op, state, keep=None):
    """An observation on renderer `r`, whose logical state is `state`: the list of arrays to compare.  `keep`: a dict of output arrays that
    outlive the renderer (the live renderer's, for LOOKAHEAD_PIN_OUTPUT)."""
    import torch
    from tinsel_amd import abi, denoise_params
    kind, p = op
    fam = state.family
    cam = _frame(fam)[0]
    size = state.size
    opt = _options(fam, size) if size else None
    dev = lambda t: t.cpu().numpy()                                                                   # noqa: E731
    if kind == "render_readback":
        o = _options(fam, size, p["depth"], p["mode"])
        out = None
        if keep is not None:
            out = keep.setdefault(size, np.empty((size[1], size[0], 4), np.float32))
        return [r.render(cam, o, output=out, passes=p["passes"]).copy()]
    if kind == "read_accum":
        return [r.read_accum()]
    if kind == "get_pass_index":
        return [np.array([r.get_pass_index()], np.uint32)]
    if kind == "present":
        return [r.present(opt, nlm_width=p["nlm"])]
    if kind == "present_image":
        return [r.present_image(_image(p["seed"], size), opt, nlm_width=p["nlm"])]
    if kind == "render_cost":
        return [r.render_cost(cam, opt, p["pass_begin"], p["passes"])]
    if kind == "features":
        planes = r.features(cam, opt, p["pass_begin"], p["passes"], which=p["mask"])
        return [planes[n] for n in sorted(planes)]
    if kind == "features_device":
        with _stream(p["stream"]):
            out = torch.empty((bin(p["mask"]).count("1"), size[1], size[0], 4), dtype=torch.float32, device="cuda")
            r.features(cam, opt, p["pass_begin"], p["passes"], which=p["mask"], out=out)
            return [dev(out)]
    if kind == "id_mattes":
        m = r.id_mattes(cam, opt, p["pass_begin"], p["passes"], slots=p["slots"])
        return [m["ids"], m["weights"], m["residual"], m["total"]]
    if kind == "id_mattes_device":
        with _stream(p["stream"]):
            ids = torch.empty((p["slots"], size[1], size[0]), dtype=torch.int32, device="cuda")
            weights = torch.empty((p["slots"] + 2, size[1], size[0]), dtype=torch.float32, device="cuda")
            r.id_mattes(cam, opt, p["pass_begin"], p["passes"], slots=p["slots"], out=(ids, weights))
            return [dev(ids), dev(weights)]
    if kind == "denoise_own":
        # the renderer's own accumulator and its own features (the accumulator is read in the default stream's order)
        if p["device"]:
            planes = None
            if p["guides"]:
                stack = torch.empty((3, size[1], size[0], 4), dtype=torch.float32, device="cuda")
                planes = r.features(cam, opt, 0, 2, out=stack)
            out = torch.empty((size[1], size[0], 4), dtype=torch.float32, device="cuda")
            return [dev(r.denoise(planes, out=out))]
        return [r.denoise(r.features(cam, opt, 0, 2) if p["guides"] else None)]
    if kind == "denoise_images":
        # caller images of another size than the frame
        z = p["size"]
        beauty = _image(p["seed"], z)
        planes = {n: _image(p["seed"] + 10*(k + 1), z) for k, n in enumerate(abi.FEATURE_NAMES)}
        params = denoise_params(radius=3, demodulate=1)
        if p["device"]:
            with _stream(p["stream"]):
                t = lambda a: torch.from_numpy(a).cuda()                                              # noqa: E731
                return [dev(r.denoise({n: t(a) for n, a in planes.items()}, params, beauty=t(beauty)))]
        return [r.denoise(planes, params, beauty=beauty)]
    if kind == "trace_rays":
        return [r.trace_rays(_inputs(fam)["rays"], p["mode"])]
    if kind == "trace_rays_device":
        with _stream(p["stream"]):
            out = dev(r.trace_rays(_device(fam, "rays"), p["mode"]))
            return [out[:, :5] if p["mode"] == "closest" else out]
    if kind == "trace_camera":
        return [r.trace_camera(cam, 50, 37, time=0.25)]
    if kind == "radiance":
        if p["device"]:
            with _stream(p["stream"]):
                return [dev(r.radiance(_device(fam, "starts"), p["depth"]))[:, :3]]
        return [r.radiance(_inputs(fam)["starts"], p["depth"])[:, :3]]
    if kind in ("gather", "gather_sh"):
        args = (rm.N_SAMPLES, p["depth"]) + ((p["order"],) if kind == "gather_sh" else ()) + (p["mode"],)
        if p["device"]:
            with _stream(p["stream"]):
                return [dev(getattr(r, kind)(_device(fam, "points"), *args))]
        return [getattr(r, kind)(_inputs(fam)["points"], *args)]
    if kind in rm.PLANE_OBSERVERS:
        if kind.endswith("_device"):
            with _stream(p["stream"]):
                return [dev(plane_call(r, rm.feature_of(kind), p, state, True))]
        return [plane_call(r, rm.feature_of(kind), p, state, False)]
    raise AssertionError(kind)


def _refused_planes(r, p, before):
    """a plane call the renderer must refuse as it is now: TinselHipError, and `out` as it was"""
    call = rm.REFUSED_PLANES[p["feature"]]
    with _stream(p.get("stream", False)):
        out = planes_out(r, p["feature"], call, before, p["device"], fill=7.0)
        _refused(lambda: plane_call(r, p["feature"], call, before, p["device"], out))
        assert bool((out == 7.0).all()), "a refused %s call wrote to its output" % p["feature"]


def _refused(call):
    import tinsel_amd
    with pytest.raises(tinsel_amd.TinselHipError):
        call()


def apply_live(r, op, before, keep):
    """A mutator, a live-only setting, a there-and-back operation or a refused call on the live renderer, whose state was `before`"""
    import torch
    from tinsel_amd import abi, denoise_params
    from tests import refit_host as rh
    kind, p = op
    fam = before.family
    cam = _frame(fam)[0]
    size = before.size
    if kind == "init":
        r.init(*p["size"])
    elif kind == "init_external":
        t = torch.full((p["size"][1], p["size"][0], 4), 7.0, dtype=torch.float32, device="cuda")      # (init zeroes it)
        keep["external"] = keep.get("external", []) + [t]
        torch.cuda.synchronize()
        r.init(p["size"][0], p["size"][1], accum_tensor=t)
    elif kind == "set_pass_index":
        r.set_pass_index(p["index"])
    elif kind == "render":
        r.render(cam, _options(fam, size, p["depth"], p["mode"]), passes=p["passes"], readback=False)
    elif kind == "render_async":
        r.render_async(cam, _options(fam, size, p["depth"], p["mode"]), passes=p["passes"], stream=None)
    elif kind == "write_accum":
        r.write_accum(_image(p["seed"], size), p["next_pass"])
    elif kind == "set_shard":
        r.set_shard(p["rank"], p["world"], p["tile"])
    elif kind == "set_russian_roulette":
        r.set_russian_roulette(p["start"])
    elif kind == "set_probe_sampling":
        r.set_probe_sampling(p["mode"])
    elif kind == "update_scene":
        assert r.update_scene(_scene(before.scene), _scene(("pack", "anim_cornell_%d" % p["frame"])))
    elif kind == "refit_mesh":
        # (positions, and normals where the op gives a seed, always made from the pack's own arrays: None keeps what the mesh has)
        r.refit_mesh(*rm.refit_arrays(("refit", rm.FAMILIES[fam]["pack"], float(p["amount"]), p["normals"])))
    elif kind == "set_pipeline":
        r.set_pipeline(getattr(abi, PIPELINE[p["pipeline"]]))
    elif kind == "set_tuning":
        r.set_tuning(abi.Tuning(**p["fields"]))
    elif kind == "set_batch_paths":
        r.set_batch_paths(p["paths"])
    elif kind == "reserve":
        r.reserve(p["passes"], p["depth"])
    elif kind == "set_lookahead":
        r.set_lookahead(p["mode"])
    elif kind == "set_counters":
        r.enable_kernel_timing(p["timing"])
        r.set_detail_counters(p["detail"])
    elif kind == "bvh_there_and_back":
        r.set_mesh_bvh(abi.BVH_LBVH if p["mode"] == "lbvh" else abi.BVH_PLOC)
        r.set_mesh_bvh(abi.BVH_REFERENCE)
    elif kind == "rebuild_there_and_back":
        r.rebuild_scene()
        r.rebuild_scene(rh.scene_nodes(rm.pack_bytes(before.scene)))
    elif kind == "fast_there_and_back":
        r.set_arithmetic(abi.ARITH_FAST)
        assert r.trace_rays(_inputs(fam)["rays"], "closest").shape == (rm.N_RAYS,)
        r.set_arithmetic(abi.ARITH_EXACT)
    elif kind == "refused_render_dirty":
        blob = rm.pack_bytes(before.scene)
        start, end = rh.transforms(blob, 0)
        r.set_primitive_transform(0, start, end)                        # a move (to where it is): the scene BVH counts as stale
        _refused(lambda: r.render(cam, _options(fam, size, 3), passes=1, readback=False))
        r.rebuild_scene(rh.scene_nodes(blob))
    elif kind in ("refused_features_size", "refused_mattes_size"):
        o = _options(fam, (size[0] + 1, size[1]))
        if kind == "refused_features_size":
            out = torch.empty((3, size[1], size[0] + 1, 4), dtype=torch.float32, device="cuda") if p["device"] else None
            _refused(lambda: r.features(cam, o, 0, 1, out=out))
        else:
            out = (torch.empty((4, size[1], size[0] + 1), dtype=torch.int32, device="cuda"),
                   torch.empty((6, size[1], size[0] + 1), dtype=torch.float32, device="cuda")) if p["device"] else None
            _refused(lambda: r.id_mattes(cam, o, 0, 1, slots=4, out=out))
    elif kind == "refused_denoise_radius":
        _refused(lambda: r.denoise(beauty=_image(1, (21, 35)), params=denoise_params(radius=9)))
    elif kind == "refused_tuning":
        _refused(lambda: r.set_tuning(abi.Tuning(walk_block=100)))
    elif kind == "refused_planes_sharded":
        r.set_shard(1, 2, 16)
        _refused_planes(r, p, before)
        r.set_shard(*before.shard)
    elif kind == "refused_planes_fast":
        r.set_arithmetic(abi.ARITH_FAST)
        _refused_planes(r, p, before)
        r.set_arithmetic(abi.ARITH_EXACT)
    elif kind == "set_bake":
        r.set_tuning(abi.Tuning(bounce_share=p["share"], bounce_bake=p["mode"]))
    else:
        raise AssertionError(kind)


def fresh(state, level="full"):
    """a fresh renderer brought to `state` by renderer_model.replay: default tuning, pipeline AUTO, no look-ahead, nothing reserved"""
    import tinsel_amd
    cam = _frame(state.family)[0]
    r = None
    for step in rm.replay(state, level):
        what, args = step[0], step[1:]
        if what == "create":
            r = tinsel_amd.create_gpu_renderer(_scene(args[0]))
        elif what == "init":
            r.init(*args)
        elif what == "write_accum":
            r.write_accum(_image(args[0], state.size), args[1])
        elif what == "render":
            r.render(cam, _options(state.family, state.size, args[0], args[1]), passes=args[2], readback=False)
        else:
            getattr(r, what)(*args)
    return r


def run_schedule(ops, seed=None, forget=None, report=None, at_end=None):
    """Runs a schedule on one live renderer and holds every observation to a fresh one; raises Mismatch at the first that differs.
    `forget`: the sabotage of renderer_model.Model -- what the fresh renderers are brought to is then the sabotaged model's belief, while the
    live renderer is always given the schedule's own, valid calls.  `at_end`: called with the live renderer behind the last op, before it
    is closed.  Returns (observations, seconds)."""
    import tinsel_amd
    truth, belief = rm.Model(), rm.Model(forget)
    live, keep, seen = None, {}, 0
    began = time.perf_counter()
    try:
        for step, op in enumerate(ops):
            kind = op[0]
            assert time.perf_counter() - began < SECONDS_PER_SCHEDULE, "seed %s: %d s and not done at step %d" % (seed, SECONDS_PER_SCHEDULE, step)
            before = truth.state.copy() if truth.state else None
            truth.apply(step, op)
            belief.apply(step, op)
            if kind == "create":
                live = tinsel_amd.create_gpu_renderer(_scene(truth.state.scene))
                continue
            if kind in rm.OBSERVERS:
                counted = live.stats() if kind in rm.PLANE_OBSERVERS else None
                got = observe(live, op, before, keep)
                if counted is not None and live.stats() != counted:          # (the statistics of these calls are their own)
                    raise Mismatch(step, op, "the statistics were %r and are %r" % (counted, live.stats()), ops, seed)
                # (a render with read-back is held to the state it leads to; every other observer leaves the state as it was)
                other = fresh(_without_last_render(belief.state) if kind == "render_readback" else belief.state, rm.replay_level(kind))
                try:
                    want = observe(other, op, _without_last_render(belief.state) if kind == "render_readback" else belief.state)
                    if rm.replay_level(kind) != "scene":            # (a fresh renderer for a query is never told the pass index)
                        want.append(np.array([other.get_pass_index()], np.uint32))
                        got.append(np.array([live.get_pass_index()], np.uint32))
                finally:
                    other.close()
                seen += 1
                what = _differ(got, want)
                if what:
                    raise Mismatch(step, op, what, ops, seed)
                if op[1].get("golden"):
                    _anchor(live, truth.state, got[0], step, op, ops, seed)
            else:
                apply_live(live, op, before, keep)
            if kind in rm.CHANGES_NOTHING and live.get_pass_index() != belief.state.next_pass:
                raise Mismatch(step, op, "the pass index is %d, the model's %d" % (live.get_pass_index(), belief.state.next_pass), ops, seed)
        if belief.state.size is not None and all(x[0] == belief.state.scene for x in belief.state.renders):
            other = fresh(belief.state)
            try:
                want = [other.read_accum(), np.array([other.get_pass_index()], np.uint32)]
            finally:
                other.close()
            what = _differ([live.read_accum(), np.array([live.get_pass_index()], np.uint32)], want)
            if what:
                raise Mismatch(len(ops) - 1, ("read_accum at the end", {}), what, ops, seed)
        if at_end is not None:
            at_end(live)
    finally:
        if live is not None:
            live.close()
    seconds = time.perf_counter() - began
    if report is not None:
        print("HISTORY %s: %s, %d ops, %d observations, %.2f s" % (report, ops[0][1]["scene"], len(ops), seen, seconds))
    return seen, seconds


def _without_last_render(state):
    """the state a render with read-back starts from: the model has applied it already"""
    s = state.copy()
    if s.renders:
        last = s.renders.pop()
        s.next_pass = last[6]
    return s


def _anchor(live, state, out, step, op, ops, seed):
    """the golden file's own frame on the live renderer: accumulator and per-path radiance array_equal to the committed ones"""
    g = np.load(os.path.join(rm.GOLDEN, rm.FAMILIES[state.family]["golden"] + ".golden.npz"))
    W, H = state.size
    rad = live.batch_radiance(op[1]["passes"], H, W)
    for name, got in (("accum", out), ("radiance", rad)):
        if not np.array_equal(got, g[name]):
            raise Mismatch(step, op, "the golden file's %s: %d of %d values differ" % (name, int((got != g[name]).sum()), got.size), ops, seed)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("seed", rm.ALL_SEEDS)         # (the chosen set, and the earlier set's seeds as further histories)
def test_history_leaves_no_trace(seed):
    ops = rm.schedule(seed)
    seen, seconds = run_schedule(ops, seed, report="seed %d" % seed)
    assert seen == len(rm.observations(ops)) >= 10


# -- teeth: the comparison notices a model that is wrong ------------------------------------------------------------------------------------------
# The MODEL is sabotaged, never the library's calls: the live renderer runs the schedule as written, the fresh ones are brought to what a
# forgetful model believes.  The mismatch must be reported at the first observation behind the sabotage and nowhere before.

RENDER = lambda passes, depth=4: ("render", {"depth": depth, "mode": "pathtrace", "passes": passes})          # noqa: E731
TEETH = {
    "a set_pass_index rewind": ([("create", {"scene": "cornell"}), ("init", {"size": (48, 32)}), RENDER(2), ("read_accum", {}),
                                 ("set_pass_index", {"index": 0}), RENDER(1), ("read_accum", {}), ("present", {"nlm": 0})], (4, "op"), 6),
    "an update_scene": ([("create", {"scene": "anim_cornell"}), ("init", {"size": (33, 17)}), RENDER(1), ("read_accum", {}),
                         ("update_scene", {"frame": 1}), ("init", {"size": (33, 17)}), ("set_pass_index", {"index": 0}), RENDER(2),
                         ("read_accum", {}), ("get_pass_index", {})], (4, "op"), 8),
    "that init changed the size": ([("create", {"scene": "cornell"}), ("init", {"size": (48, 32)}), RENDER(1), ("read_accum", {}),
                                    ("init", {"size": (16, 16)}), RENDER(1), ("read_accum", {}), ("present", {"nlm": 1})], (4, "size"), 6),
}
# the plane features: the model forgets an update_scene, and the first observation behind it is one of theirs
_MOVED = [("create", {"scene": "anim_cornell"}), ("init", {"size": (33, 17)}), RENDER(1), ("read_accum", {}), ("update_scene", {"frame": 1}),
          ("init", {"size": (33, 17)})]
TEETH.update({
    "an update_scene before light groups": (_MOVED + [("light_groups", {"table": "parity", "pass_begin": 5, "passes": 2}), ("get_pass_index", {})], (4, "op"), 6),
    "an update_scene before views": (_MOVED + [("views_device", {"count": 3, "pass_begin": 7, "passes": 1, "add": True, "singly": False, "seed": 2,
                                                                 "stream": True}), ("get_pass_index", {})], (4, "op"), 6),
    "an update_scene before a sample map": (_MOVED + [("sample_map", {"map": "uniform", "pass_begin": 3, "add": False, "seed": 1}),
                                                      ("get_pass_index", {})], (4, "op"), 6),
    "an update_scene before depth planes": (_MOVED + [("depth_planes_device", {"depths": (1, 2, 3, 4), "pass_begin": 2, "passes": 2, "add": False,
                                                                               "singly": True, "seed": 1, "stream": False}),
                                                      ("get_pass_index", {})], (4, "op"), 6),
})


@pytest.mark.timeout(120)
@pytest.mark.parametrize("what", sorted(TEETH))
def test_a_model_that_forgets_is_caught_at_the_first_observation_behind(what):
    ops, forget, expected = TEETH[what]
    assert [k for k in rm.observations(ops) if k > forget[0]][0] == expected
    with pytest.raises(Mismatch) as caught:
        run_schedule(ops, forget=forget)                             # (it raises at the FIRST mismatch: none before)
    print(caught.value)
    assert caught.value.step == expected
    run_schedule(ops)                                                # and the schedule itself is sound


BAKED = [("create", {"scene": "cornell"}), ("set_bake", {"mode": 1, "share": 0}), ("init", {"size": (64, 64)}), RENDER(2), ("read_accum", {}),
         ("views", {"count": 3, "pass_begin": 7, "passes": 1, "add": False, "singly": False, "seed": 1}), ("reserve", {"passes": 4, "depth": 4}),
         ("init", {"size": (64, 64)}), ("set_pass_index", {"index": 0}),
         ("render_readback", {"depth": 4, "mode": "pathtrace", "passes": 4, "golden": True})]


@pytest.mark.timeout(120)
def test_the_baked_instance_serves_a_schedule_that_asks_for_it():
    """set_bake is never an error: where nothing compiles, every schedule with it would pass on the library's own instance.  So once, on the
    scene whose plan gives the closed fused kernel, the baked instance must be installed and must have served launches -- and then its
    frame is the golden file's, bit for bit (the anchor), and every observation a fresh, unbaked renderer's."""
    from tinsel_amd import abi
    status = []
    seen, _ = run_schedule(BAKED, report="baked", at_end=lambda live: status.append(live.bake_status()))
    assert seen == len(rm.observations(BAKED)) == 3
    print(status[0])
    assert status[0]["state"] in (abi.BAKE_COMPILED, abi.BAKE_FROM_CACHE), status[0]
    assert status[0]["launches"] > 0, status[0]


# -- groups -----------------------------------------------------------------------------------------------------------------------------------------

def _group(family, n, tile, monkeypatch):
    import torch
    from tinsel_amd import HipRendererGroup
    if torch.cuda.device_count() < n:
        monkeypatch.setenv("TINSEL_HIP_GROUP_ONE_DEVICE", "1")
    return HipRendererGroup(_scene(("pack", rm.FAMILIES[family]["pack"])), n, tile)


def _group_pass_index(grp, index):
    """every member's next pass (a group has no entry of its own for it: its members keep the index)"""
    for k in range(grp.num_gpus):
        assert grp._L.tinsel_hip_set_pass_index(grp._L.tinsel_hip_group_member(grp._h, k), index) == 0


def _group_observe(grp, op, state):
    cam = _frame(state.family)[0]
    kind, p = op
    if kind == "present":
        return grp.present(_options(state.family, state.size), nlm_width=p["nlm"])
    return grp.render(cam, _options(state.family, state.size, p["depth"], p["mode"]), passes=p["passes"])


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n,tile,family,seed", rm.GROUPS)
def test_group_history_leaves_no_trace(n, tile, family, seed, monkeypatch):
    """The live group against a fresh group of the same members and tile.  Under the one-device validation switch the sum runs in rank order
    and is deterministic: bit for bit.  Over real devices the reduce's order is RCCL's: rtol 1e-5, atol 1e-6, as tests/test_gpu_group.py."""
    import torch
    exact = torch.cuda.device_count() < n
    print("group of %d, tile %d: %s" % (n, tile, "one-device arm, bit for bit" if exact else "real devices, rtol 1e-5 atol 1e-6"))
    ops = [("create", {"scene": family})] + rm.group_schedule(seed)
    model = rm.Model()
    cam = _frame(family)[0]
    keep, seen, began = {}, 0, time.perf_counter()
    live = _group(family, n, tile, monkeypatch)
    try:
        for step, op in enumerate(ops):
            kind, p = op
            before = model.state.copy() if model.state else None
            model.apply(step, op)
            if kind == "create":
                continue
            if kind == "init":
                live.init(*p["size"])
            elif kind == "set_lookahead":
                live.set_lookahead(p["mode"])
            elif kind == "render":
                live.render(cam, _options(family, before.size, p["depth"], p["mode"]), passes=p["passes"], readback=False)
            elif kind in ("render_readback", "present"):
                if kind == "present":
                    got = _group_observe(live, op, before)
                else:
                    out = keep.setdefault(before.size, np.empty((before.size[1], before.size[0], 4), np.float32))
                    got = live.render(cam, _options(family, before.size, p["depth"], p["mode"]), output=out, passes=p["passes"]).copy()
                state = _without_last_render(model.state) if kind == "render_readback" else model.state
                other = _group(family, n, tile, monkeypatch)
                try:
                    other.init(*state.size)
                    for r in state.renders:
                        _group_pass_index(other, r[6])
                        other.render(cam, _options(family, state.size, r[4], r[5]), passes=r[7], readback=False)
                    _group_pass_index(other, state.next_pass)
                    want = _group_observe(other, op, state)
                finally:
                    other.close()
                seen += 1
                if exact:
                    what = _differ([got], [want])
                    if what:
                        raise Mismatch(step, op, what, ops, seed)
                else:
                    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6, err_msg="seed %d, step %d, op %r\n%r" % (seed, step, op, ops[:step + 1]))
            else:
                raise AssertionError(kind)
    finally:
        live.close()
    print("HISTORY group %d x tile %d: %s, %d ops, %d observations, %.2f s" % (n, tile, family, len(ops), seen, time.perf_counter() - began))
    assert seen >= 8

"""A model of what a renderer's history may change, and seeded histories of API calls to hold a live renderer to it.

Host only: nothing here touches the GPU, and nothing of the library is loaded at import.  tests/test_renderer_model.py checks the committed
schedules on the CPU (what they cover), tests/test_gpu_histories.py runs them (DESIGN.md "What a renderer's history may not change").

An op is a Python literal `(kind, {parameter: value})`; a schedule is a list of them whose first op is `("create", {"scene": name})`.

The LOGICAL STATE (class State) is what a caller may rely on: the scene (as a key pack_bytes() turns into pack bytes), the frame size, the
accumulator's contents -- the array given to write_accum, if any, and the renders since the last init, each with the settings it ran under --,
the next pass index, the shard, the roulette start, the probe sampling mode, the arithmetic arm and whether a primitive was moved without a
rebuild.  Everything else a renderer remembers is a cache.  LIVE_ONLY ops set what the project documents as bit-neutral: the fresh renderer
never gets them (set_bake, the bake mode of the closed fused kernel, among them).  THERE_AND_BACK and REFUSED ops leave the logical state
as it was.  `replay(state)` is the shortest route that brings a fresh renderer to a state: a recipe, it launches nothing.

The PLANE_OBSERVERS -- light groups, view batches, sample maps, depth planes, each through its host and its device entry -- need the frame
but not its contents, keep renderer-lifetime buffers, seed tables and fences of their own, and refuse a sharded renderer and the
tolerance arm: the builder sets the shard back in front of one."""
import copy
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

SIZES = ((16, 16), (33, 17), (48, 32), (50, 37), (96, 64))          # ragged against the 16x16, 32x8 and 64-wide tiles
DEPTHS = (2, 3, 4, 6)
ANIM_FRAMES = 4
DEFAULT_SHARD = (0, 1, 32)
SHARDS = ((1, 2, 16), (0, 2, 32), (2, 3, 16), (0, 1, 32))
N_RAYS, N_STARTS, N_POINTS, N_SAMPLES = 4096, 2048, 256, 8
MAX_OPS, MAX_SCHEDULES = 44, 16
MAX_REPLAY_RENDERS, MAX_REPLAY_PASSES = 4, 8
SEED_TABLE_AHEAD = 1024                                             # render_impl's kSeedsAhead (tn_host_batch.h)

# scene family -> (first pack, has a golden file, supports update_scene / refit_mesh / set_probe_sampling)
FAMILIES = {
    "anim_cornell": dict(pack="anim_cornell_0", golden=None, update=True, refit=False, probe=False),
    "ajax_standin_96": dict(pack="ajax_standin_96", golden="ajax_standin_96", update=False, refit=True, probe=False),
    "features_probe": dict(pack="features_probe", golden="features_probe", update=False, refit=False, probe=True),
    "motionblur": dict(pack="motionblur", golden="motionblur", update=False, refit=False, probe=False),
    "glass": dict(pack="glass", golden="glass", update=False, refit=False, probe=False),
    "cornell": dict(pack="cornell", golden="cornell", update=False, refit=False, probe=False),
}
FAMILY_ORDER = ("anim_cornell", "ajax_standin_96", "features_probe", "motionblur", "glass", "cornell")
# the golden files' frames: (width, height, max_depth, passes), checked against the files by tests/test_renderer_model.py
GOLDEN_FRAMES = {"ajax_standin_96": (96, 96, 4, 3), "features_probe": (96, 64, 6, 4), "motionblur": (64, 64, 4, 3),
                 "glass": (64, 64, 12, 3), "cornell": (64, 64, 4, 4)}
REFITS = ((0.05, None), (0.02, 7), (0.0, 0))                        # (displacement, seed of new normals | None: kept); the last is the way back

MUTATORS = ("init", "init_external", "set_pass_index", "render", "render_async", "write_accum", "set_shard", "set_russian_roulette",
            "set_probe_sampling", "update_scene", "refit_mesh")
LIVE_ONLY = ("set_pipeline", "set_tuning", "set_batch_paths", "reserve", "set_lookahead", "set_counters", "set_bake")
THERE_AND_BACK = ("bvh_there_and_back", "rebuild_there_and_back", "fast_there_and_back")
REFUSED = ("refused_render_dirty", "refused_features_size", "refused_mattes_size", "refused_denoise_radius", "refused_tuning",
           "refused_planes_sharded", "refused_planes_fast")
# the four calls that give planes of the beauty, each with a host and a `_device` entry: they refuse a sharded renderer and the tolerance arm
PLANE_FEATURES = ("light_groups", "views", "sample_map", "depth_planes")
PLANE_OBSERVERS = tuple(f + e for f in PLANE_FEATURES for e in ("", "_device"))
OBSERVERS = ("render_readback", "read_accum", "get_pass_index", "present", "present_image", "render_cost", "features", "features_device",
             "id_mattes", "id_mattes_device", "denoise_own", "denoise_images", "trace_rays", "trace_rays_device", "trace_camera",
             "radiance", "gather", "gather_sh") + PLANE_OBSERVERS
ALL_KINDS = ("create",) + MUTATORS + LIVE_ONLY + THERE_AND_BACK + REFUSED + OBSERVERS
# observers that only read the scene (a fresh renderer needs no frame), and those that need the frame and the shard but not its contents
SCENE_OBSERVERS = ("trace_rays", "trace_rays_device", "trace_camera", "radiance", "gather", "gather_sh", "denoise_images")
FRAME_OBSERVERS = ("render_cost", "features", "features_device", "id_mattes", "id_mattes_device") + PLANE_OBSERVERS
# ops after which get_pass_index() is checked at once: they must change nothing
CHANGES_NOTHING = tuple(k for k in OBSERVERS if k != "render_readback") + THERE_AND_BACK + REFUSED

PIPELINES = ("auto", "wavefront", "split", "paired", "megakernel")
TUNINGS = ({"grid_mult": 4, "walk_lds_stack": 2}, {"shade_sorted": 1, "accumulate": 2}, {"overlap": 1, "walk_single": 0},
           {"repack": 1, "tail_split": 1, "tail_share": 0.4, "tail_divide": 8}, {"accumulate": 3, "overlap": 0, "repack": 0, "shade_sorted": 0},
           {"tail_split": 0, "grid_mult": 16, "accumulate": 1}, {})
TUNING_FIELDS = ("grid_mult", "accumulate", "overlap", "shade_sorted", "repack", "tail_split", "walk_lds_stack", "walk_single", "bounce_share",
                 "bounce_bake")
# what the plane observers draw (tests/test_gpu_histories.py makes the tables, cameras and maps from these names)
GROUP_TABLES = ("one", "parity", "eight")                           # -> (groups G, env_group): see group_table
VIEW_COUNTS = (1, 3, 6)
SAMPLE_MAPS = ("uniform", "random", "crop", "zeros")
PLANE_DEPTHS = ((1,), (1, 2, 3, 4), (2, 6), tuple(range(1, 17)))
PLANE_PASSES = {"light_groups": (0, 5, 1200), "views": (0, 7, 1300), "sample_map": (0, 3, 1400), "depth_planes": (0, 2, 1600)}
BAKE_MODES, BAKE_SHARES = (1, 0, -1), (0, -1)
# the call a refused_planes_* op makes, per feature
REFUSED_PLANES = {"light_groups": dict(table="parity", pass_begin=0, passes=1),
                  "views": dict(count=3, pass_begin=0, passes=1, add=False, singly=False, seed=1),
                  "sample_map": dict(map="uniform", pass_begin=0, add=False, seed=1),
                  "depth_planes": dict(depths=(1, 2, 3, 4), pass_begin=0, passes=1, add=False, singly=False, seed=1)}


def feature_of(kind):
    """the plane feature of an observer kind, or None"""
    f = kind[:-len("_device")] if kind.endswith("_device") else kind
    return f if f in PLANE_FEATURES else None


def group_table(name, primitives):
    """(group of every primitive, env_group, G) of a light-group table, from the scene's primitive count alone: "one" puts every primitive
    in group 0; "parity" primitive i in group i % 2 and the environment in 1; "eight" primitive i in group i % 8, every seventh in none."""
    if name == "one":
        return [0]*primitives, 0, 1
    if name == "parity":
        return [i % 2 for i in range(primitives)], 1, 2
    assert name == "eight", name
    return [-1 if i % 7 == 6 else i % 8 for i in range(primitives)], -1, 8


def supports(family, kind):
    f = FAMILIES[family]
    return {"update_scene": f["update"], "refit_mesh": f["refit"], "set_probe_sampling": f["probe"]}.get(kind, True)


# -- the logical state -------------------------------------------------------------------------------------------------------------------

class State:
    """What a caller may rely on.  `renders`: (scene, shard, roulette, probe, depth, mode, first_pass, passes) of every render since the
    last init / write_accum, in order; `written`: (seed, next_pass) of the array write_accum gave, or None."""

    def __init__(self, family):
        self.family = family
        self.scene = ("pack", FAMILIES[family]["pack"])
        self.size = None
        self.written = None
        self.renders = []
        self.next_pass = 0
        self.shard = DEFAULT_SHARD
        self.roulette = 0
        self.probe = 0
        self.arith = 0
        self.dirty = False

    def copy(self):
        return copy.deepcopy(self)

    def replay_cost(self):
        return len(self.renders), sum(r[7] for r in self.renders if r[5] == "pathtrace")


class Model:
    """Applies ops to a State.  `forget`: (step, what) sabotages the model on purpose (the teeth of tests/test_gpu_histories.py): at op
    number `step` it forgets the "op" altogether, or, of an init, only that the "size" changed."""

    def __init__(self, forget=None):
        self.state = None
        self.forget = forget

    def apply(self, step, op):
        kind, p = op
        if kind == "create":
            assert self.state is None and step == 0
            self.state = State(p["scene"])
            return
        s = self.state
        assert s is not None, "a schedule starts with create"
        assert kind in ALL_KINDS, kind
        assert supports(s.family, kind), "%s does not support %s" % (s.family, kind)
        if self.forget and self.forget[0] == step and self.forget[1] == "op":
            return
        if kind in ("init", "init_external"):
            if not (self.forget and self.forget[0] == step and self.forget[1] == "size"):
                s.size = tuple(p["size"])
            s.written, s.renders = None, []
        elif kind == "set_pass_index":
            s.next_pass = int(p["index"])
        elif kind in ("render", "render_async", "render_readback"):
            assert s.size is not None and not s.dirty
            assert all(r[0] == s.scene for r in s.renders), "one frame, one scene: init after the scene changes"
            s.renders.append((s.scene, s.shard, s.roulette, s.probe, int(p["depth"]), p["mode"], s.next_pass, int(p["passes"])))
            if p["mode"] == "pathtrace":                # (a NORMALS render overwrites and leaves the pass index: render_impl)
                s.next_pass += int(p["passes"])
            n, passes = s.replay_cost()
            assert n <= MAX_REPLAY_RENDERS and passes <= MAX_REPLAY_PASSES, "a fresh replay stays short: init more often"
        elif kind == "write_accum":
            assert s.size is not None
            s.written, s.renders = (int(p["seed"]), int(p["next_pass"])), []
            s.next_pass = int(p["next_pass"])
        elif kind == "set_shard":
            s.shard = (int(p["rank"]), int(p["world"]), int(p["tile"]))
        elif kind == "set_russian_roulette":
            s.roulette = int(p["start"])
        elif kind == "set_probe_sampling":
            s.probe = int(p["mode"])
        elif kind == "update_scene":
            assert s.scene[0] == "pack" and 0 <= int(p["frame"]) < ANIM_FRAMES
            s.scene = ("pack", "anim_cornell_%d" % int(p["frame"]))
        elif kind == "refit_mesh":
            kept = s.scene[3] if s.scene[0] == "refit" else None
            s.scene = ("refit", FAMILIES[s.family]["pack"], float(p["amount"]), p["normals"] if p["normals"] is not None else kept)
        else:
            # live-only settings, there-and-back operations, refused calls and the plain observers: the logical state stays
            if kind in FRAME_OBSERVERS + ("read_accum", "present", "present_image", "denoise_own", "reserve") or kind in REFUSED[1:3] + REFUSED[5:7]:
                assert s.size is not None, kind
            if kind in PLANE_OBSERVERS:
                assert s.shard[1] == 1 and s.arith == 0, "%s refuses a sharded renderer and the tolerance arm" % kind
            if kind in OBSERVERS and replay_level(kind) == "full":
                assert all(r[0] == s.scene for r in s.renders), "one frame, one scene: init after the scene changes"


def replay(state, level="full"):
    """The shortest route to `state` for a fresh renderer, as a list of (method, arguments): create from the state's scene; the shard, the
    roulette start and the probe mode; init, or init + write_accum; then per recorded render set_pass_index + render(readback=False) under
    the settings it ran with; at the end the state's own settings and pass index where the last render left others.  level "scene" stops
    before init (queries), "frame" after it (features, mattes, cost)."""
    steps = [("create", state.scene)]
    now = {"shard": DEFAULT_SHARD, "roulette": 0, "probe": 0, "pass": 0}

    def settings(shard, roulette, probe):
        if shard != now["shard"]:
            steps.append(("set_shard",) + tuple(shard))
        if roulette != now["roulette"]:
            steps.append(("set_russian_roulette", roulette))
        if probe != now["probe"]:
            steps.append(("set_probe_sampling", probe))
        now.update(shard=shard, roulette=roulette, probe=probe)

    if level == "full" and state.size is not None:
        first = state.renders[0] if state.renders else None
        settings(*(first[1:4] if first else (state.shard, state.roulette, state.probe)))
        steps.append(("init",) + tuple(state.size))
        if state.written is not None:
            steps.append(("write_accum",) + tuple(state.written))
            now["pass"] = state.written[1]
        for scene, shard, roulette, probe, depth, mode, first_pass, passes in state.renders:
            assert scene == state.scene
            settings(shard, roulette, probe)
            if first_pass != now["pass"]:
                steps.append(("set_pass_index", first_pass))
            steps.append(("render", depth, mode, passes))
            now["pass"] = first_pass + (passes if mode == "pathtrace" else 0)
    settings(state.shard, state.roulette, state.probe)
    if level == "frame" and state.size is not None:
        steps.append(("init",) + tuple(state.size))
    if level != "scene" and state.next_pass != now["pass"]:
        steps.append(("set_pass_index", state.next_pass))
    return steps


def replay_level(kind):
    return "scene" if kind in SCENE_OBSERVERS else "frame" if kind in FRAME_OBSERVERS else "full"


# -- scenes as pack bytes -----------------------------------------------------------------------------------------------------------------

_PACKS = {}


def displace(pos, amount):
    """the deformation tests/test_gpu_refit.py uses: a ripple in y and a stretch in x that leaves the original boxes"""
    import numpy as np
    p = pos.astype(np.float32).copy()
    if not amount:                                       # the way back: the pack's own positions, bit for bit
        return p
    p[:, 1] += (amount*np.sin(7.0*p[:, 0].astype(np.float64) + 3.0*p[:, 2].astype(np.float64))).astype(np.float32)
    p[:, 0] *= np.float32(1.0 + 4.0*amount)
    return p


def new_normals(normals, seed):
    """unit normals perturbed by N(0, 0.3^2) per component, renormalised in fp32 (seed 0: the pack's own)"""
    import numpy as np
    if not seed:
        return normals.astype(np.float32).copy()
    n = (normals + np.random.default_rng(seed).normal(0.0, 0.3, normals.shape)).astype(np.float32)
    ln = np.sqrt((n[:, 0]*n[:, 0] + n[:, 1]*n[:, 1]) + n[:, 2]*n[:, 2])
    return (n/ln[:, None]).astype(np.float32)


def mesh_primitive(blob):
    from tests import refit_host as rh
    return rh.mesh_prims(blob)[0]


def refit_arrays(scene):
    """(primitive, positions, normals | None) a refit_mesh call that leads to the scene key `scene` passes: always from the pack's own arrays"""
    from tests import refit_host as rh
    _, name, amount, nseed = scene
    blob = bytearray(pack_bytes(("pack", name)))
    prim = mesh_primitive(blob)
    pos = rh.mesh_views(blob, prim)[0].copy()
    nrm = rh.mesh_normals(blob, prim).copy()
    return prim, displace(pos, amount), (None if nseed is None else new_normals(nrm, nseed))


def pack_bytes(scene):
    """The pack bytes of a scene key: ("pack", name) is the committed file; ("refit", name, amount, normals seed) is that pack rewritten on
    the host by tests/refit_host.py (pinned to the reference's builder by tests/test_refit_host.py)."""
    if scene not in _PACKS:
        if scene[0] == "pack":
            with open(os.path.join(GOLDEN, scene[1] + ".pack"), "rb") as fh:
                _PACKS[scene] = fh.read()
        else:
            from tests import refit_host as rh
            prim, pos, nrm = refit_arrays(scene)
            blob = bytearray(pack_bytes(("pack", scene[1])))
            rh.refit_pack(blob, prim, pos, nrm)
            _PACKS[scene] = bytes(blob)
    return _PACKS[scene]


# -- the generator --------------------------------------------------------------------------------------------------------------------------

class _Rng:
    """splitmix64: the same draws in every process and on every machine (nothing of `random`'s algorithms is relied on)"""

    def __init__(self, seed):
        self.x = (int(seed)*0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) & 0xFFFFFFFFFFFFFFFF

    def next(self):
        self.x = (self.x + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        z = self.x
        z = ((z ^ (z >> 30))*0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 27))*0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        return z ^ (z >> 31)

    def below(self, n):
        return self.next() % n

    def pick(self, seq):
        return seq[self.below(len(seq))]

    def shuffled(self, seq):
        out = list(seq)
        for i in range(len(out) - 1, 0, -1):
            j = self.below(i + 1)
            out[i], out[j] = out[j], out[i]
        return out


class _Builder:
    """Draws valid ops: the model says what the state is, so that every call a schedule makes is one the library accepts (or, for the
    refused kinds, one it documents as refused)."""

    def __init__(self, seed):
        self.rng = _Rng(seed)
        self.family = FAMILY_ORDER[seed % len(FAMILY_ORDER)]
        self.side_stream = seed % 3 == 0                 # device entries on a non-default stream in these schedules
        self.model = Model()
        self.ops = []
        self.small_batches = False
        self.lookahead = 0
        self.bake = None                                 # (mode, share) of the set_bake in force: a set_tuning drops it
        self.reserve = self._anchor_reserve()
        self.emit("create", scene=self.family)

    # what the golden anchor at the end may need
    def _anchor_reserve(self):
        return 8 if FAMILIES[self.family]["golden"] else 0

    def room(self):
        return MAX_OPS - self.reserve - len(self.ops)

    def emit(self, kind, **p):
        op = (kind, p)
        self.model.apply(len(self.ops), op)
        self.ops.append(op)
        if kind == "set_batch_paths":
            self.small_batches = p["paths"] < (1 << 20)
        if kind in ("set_tuning", "set_bake"):
            self.small_batches = False                   # (set_tuning takes the struct's batch_paths: the default)
            self.bake = (p["mode"], p["share"]) if kind == "set_bake" else None
        if kind == "set_lookahead":
            self.lookahead = p["mode"]

    @property
    def s(self):
        return self.model.state

    # -- mutators
    def init(self, size=None, external=False):
        if size is None:
            # a schedule both shrinks and grows: whichever it has not done yet comes first
            areas = [p["size"][0]*p["size"][1] for k, p in self.ops if k in INITS]
            steps = list(zip(areas, areas[1:]))
            smaller = [z for z in SIZES if areas and z[0]*z[1] < areas[-1]]
            larger = [z for z in SIZES if areas and z[0]*z[1] > areas[-1]]
            if smaller and not any(a > b for a, b in steps):
                size = self.rng.pick(smaller)
            elif larger and not any(a < b for a, b in steps):
                size = self.rng.pick(larger)
            else:
                size = self.rng.pick(SIZES)
        self.emit("init_external" if external else "init", size=tuple(size))

    def frame(self):
        """a frame to observe: an init if there is none"""
        if self.s.size is None:
            self.init()

    def render(self, kind="render", depth=None, mode="pathtrace", passes=None):
        self.frame()
        passes = 1 if mode == "normals" else (passes or 1 + self.rng.below(3))
        n, total = self.s.replay_cost()
        if n + 1 > MAX_REPLAY_RENDERS or total + passes > MAX_REPLAY_PASSES or any(r[0] != self.s.scene for r in self.s.renders):
            self.init(self.s.size)
        p = dict(depth=depth or self.rng.pick(DEPTHS), mode=mode, passes=passes)
        if kind == "render_async":
            p["stream"] = False
        self.emit(kind, **p)

    def content(self):
        """something in the accumulator to look at"""
        self.frame()
        if not self.s.renders and self.s.written is None:
            self.render()

    def mutate(self, kind):
        r = self.rng
        if kind == "init":
            self.init()
        elif kind == "init_external":
            self.init(external=True)
        elif kind == "set_pass_index":
            self.emit(kind, index=r.pick((0, 1, 5, 17, 300, 1023)))
        elif kind in ("render", "render_async"):
            self.render(kind, mode="normals" if r.below(4) == 0 else "pathtrace")
        elif kind == "write_accum":
            self.frame()
            self.emit(kind, seed=1 + r.below(3), next_pass=r.pick((0, 2, 9)))
        elif kind == "set_shard":
            rank, world, tile = r.pick([x for x in SHARDS if x != self.s.shard])
            self.emit(kind, rank=rank, world=world, tile=tile)
        elif kind == "set_russian_roulette":
            self.emit(kind, start=r.pick([x for x in (0, 1, 2, 3) if x != self.s.roulette]))
        elif kind == "set_probe_sampling":
            self.emit(kind, mode=1 - self.s.probe)
        elif kind == "update_scene":
            now = int(self.s.scene[1][-1])
            self.emit(kind, frame=(now + 1) % ANIM_FRAMES if r.below(4) else (now - 1) % ANIM_FRAMES)
        elif kind == "refit_mesh":
            amount, nseed = r.pick(REFITS[:2])
            self.emit(kind, amount=amount, normals=nseed)
        else:
            raise AssertionError(kind)
        if kind in ("update_scene", "refit_mesh") and self.s.renders:
            self.init(self.s.size)                       # one frame, one scene: what was rendered before is another scene's

    def live_only(self, kind):
        r = self.rng
        if kind == "set_pipeline":
            self.emit(kind, pipeline=r.pick(PIPELINES))
        elif kind == "set_tuning":
            self.emit(kind, fields=dict(r.pick(TUNINGS)))
        elif kind == "set_batch_paths":
            self.emit(kind, paths=r.pick((1024, 1536, 4096)))
        elif kind == "reserve":
            self.frame()
            self.emit(kind, passes=1 + r.below(4), depth=r.pick(DEPTHS + (8,)))
        elif kind == "set_lookahead":
            self.emit(kind, mode=r.pick([m for m in (0, 1, 2) if m != self.lookahead]))
        elif kind == "set_counters":
            self.emit(kind, timing=bool(r.below(2)), detail=bool(r.below(2)))
        elif kind == "set_bake":
            self.emit(kind, mode=r.pick(BAKE_MODES), share=r.pick(BAKE_SHARES))
        else:
            raise AssertionError(kind)

    def neutral(self, kind):
        """a there-and-back operation or a refused call"""
        if kind == "bvh_there_and_back":
            self.emit(kind, mode=self.rng.pick(("lbvh", "ploc")))
        elif kind in ("refused_planes_sharded", "refused_planes_fast"):
            self.frame()
            p = dict(feature=self.rng.pick(PLANE_FEATURES), device=bool(self.rng.below(2)))
            if p["device"]:
                p["stream"] = self.side_stream
            self.emit(kind, **p)
        elif kind in ("refused_features_size", "refused_mattes_size"):
            self.frame()
            self.emit(kind, device=bool(self.rng.below(2)))
        elif kind == "refused_render_dirty":
            self.frame()
            self.emit(kind)
        else:
            self.emit(kind)

    # -- observers
    def observe(self, kind, **over):
        r = self.rng
        stream = self.side_stream
        if kind == "render_readback":
            self.render(kind, **over)
            return
        if kind in PLANE_OBSERVERS and self.s.shard[1] > 1:              # (they refuse a sharded renderer)
            self.emit("set_shard", rank=DEFAULT_SHARD[0], world=DEFAULT_SHARD[1], tile=DEFAULT_SHARD[2])
        if kind in ("read_accum", "present", "present_image", "denoise_own"):
            self.content()
        elif kind in FRAME_OBSERVERS:
            self.frame()
        if kind == "present":
            p = dict(nlm=r.below(3))
        elif kind == "present_image":
            p = dict(nlm=r.below(2), seed=1 + r.below(3))
        elif kind == "render_cost":
            p = dict(pass_begin=r.pick((0, 3, 2000)), passes=1 + r.below(2))
        elif kind in ("features", "features_device"):
            p = dict(mask=1 + r.below(7), pass_begin=r.pick((0, 4, 1500)), passes=1 + r.below(3))
        elif kind in ("id_mattes", "id_mattes_device"):
            p = dict(slots=r.pick((1, 4, 8)), pass_begin=r.pick((0, 6, 1100)), passes=1 + r.below(3))
        elif kind == "denoise_own":
            p = dict(guides=bool(r.below(3)), device=bool(r.below(2)))
        elif kind == "denoise_images":
            p = dict(size=r.pick(((40, 24), (21, 35))), seed=1 + r.below(3), device=bool(r.below(2)))
        elif kind in ("trace_rays", "trace_rays_device"):
            p = dict(mode=r.pick(("closest", "occluded")))
        elif kind == "radiance":
            p = dict(depth=r.pick(DEPTHS), device=bool(r.below(2)))
        elif kind == "gather":
            p = dict(mode=r.pick(("cosine", "sphere")), depth=r.pick(DEPTHS[:3]), device=bool(r.below(2)))
        elif kind == "gather_sh":
            p = dict(order=r.below(3), mode=r.pick(("cosine", "sphere")), depth=r.pick(DEPTHS[:3]), device=bool(r.below(2)))
        elif feature_of(kind) == "light_groups":
            p = dict(table=r.pick(GROUP_TABLES), pass_begin=r.pick(PLANE_PASSES["light_groups"]), passes=1 + r.below(2))
        elif feature_of(kind) == "views":
            p = dict(count=r.pick(VIEW_COUNTS), pass_begin=r.pick(PLANE_PASSES["views"]), passes=1 + r.below(2), add=bool(r.below(2)),
                     singly=bool(r.below(2)), seed=1 + r.below(3))
        elif feature_of(kind) == "sample_map":
            p = dict(map=r.pick(SAMPLE_MAPS), pass_begin=r.pick(PLANE_PASSES["sample_map"]), add=bool(r.below(2)), seed=1 + r.below(3))
        elif feature_of(kind) == "depth_planes":
            p = dict(depths=r.pick(PLANE_DEPTHS), pass_begin=r.pick(PLANE_PASSES["depth_planes"]), passes=1 + r.below(2), add=bool(r.below(2)),
                     singly=bool(r.below(2)), seed=1 + r.below(3))
        else:
            p = {}
        p.update(over)
        if kind.endswith("_device") or p.get("device"):
            p["stream"] = stream
        self.emit(kind, **p)

    # -- the sequences tests/test_renderer_model.py asks for, each drawn into some schedules
    def motif_shrink_grow(self):
        big, small, again = self.rng.pick(((96, 64), (50, 37))), self.rng.pick(((33, 17), (16, 16))), self.rng.pick(((96, 64), (48, 32)))
        for size in (big, small, again):
            self.init(size)
            self.render()
            self.observe("present", nlm=1 + self.rng.below(2))
            self.observe("denoise_own")

    def motif_depth_and_pipeline(self):
        self.init()
        self.render(depth=6)
        self.render(depth=2, passes=1)
        self.render(depth=4, passes=1)
        self.emit("set_pipeline", pipeline=self.rng.pick(PIPELINES[1:]))
        self.render(depth=3, passes=1)
        self.observe("read_accum")

    def motif_shared_buffers(self):
        self.init()
        self.render(passes=1)
        self.observe(self.rng.pick(("radiance", "gather", "gather_sh")))
        self.render(passes=1)
        self.observe(self.rng.pick(("features", "id_mattes", "features_device", "id_mattes_device")), pass_begin=self.s.next_pass + 40)
        self.render(passes=1)
        self.observe("read_accum")

    def motif_seed_table(self):
        self.init()
        self.emit("set_pass_index", index=0)
        self.render(passes=2)
        self.emit("set_pass_index", index=SEED_TABLE_AHEAD + 1 + self.rng.below(50))
        self.render(passes=1)
        self.emit("set_pass_index", index=1 + self.rng.below(3))
        self.render(passes=2)
        self.observe("render_readback", passes=1)

    def motif_shard(self):
        self.init()
        self.render(passes=1)
        self.mutate("set_shard")
        self.render(passes=1)
        self.observe("read_accum")
        self.observe("features", mask=7)

    def motif_lookahead(self):
        self.init()
        self.emit("set_lookahead", mode=1 + self.rng.below(2))
        self.observe("render_readback", depth=4, passes=1)
        self.observe("render_readback", depth=4, passes=1)
        self.observe("render_readback", depth=2, passes=1)       # a miss: the options changed
        self.observe("present", nlm=self.rng.below(2))
        self.observe("render_readback", depth=2, passes=1)

    def _entry(self, feature):
        return feature + ("_device" if self.rng.below(2) else "")

    def motif_planes_shrink_grow(self):
        """record and output buffers that only grow: every plane feature at a big frame, a smaller one and a bigger one again"""
        big, small, again = self.rng.pick(((96, 64), (50, 37))), self.rng.pick(((33, 17), (16, 16))), self.rng.pick(((96, 64), (48, 32)))
        # (the last frame asks for more planes and passes than the first, so that it needs the largest buffers of the three whatever its size)
        few = {"light_groups": dict(table="one", passes=1), "views": dict(count=1, passes=1),
               "sample_map": dict(map="crop"), "depth_planes": dict(depths=self.rng.pick(PLANE_DEPTHS[:1] + PLANE_DEPTHS[2:3]), passes=1)}
        many = {"light_groups": dict(table="eight", passes=2), "views": dict(count=6, passes=2), "sample_map": dict(map="uniform"),
                "depth_planes": dict(depths=PLANE_DEPTHS[3], passes=2)}
        for size, over in ((big, few), (small, few), (again, many)):
            self.init(size)
            self.render(passes=1)
            for f in self.rng.shuffled(PLANE_FEATURES):
                self.observe(self._entry(f), **over[f])
        self.observe("render_readback", passes=1)

    def motif_planes_between_renders(self):
        """a plane call at a pass of its own between two renders of one frame: its seeds, records and fence, and the path buffers it borrows"""
        self.init()
        self.render(passes=1)
        for k, f in enumerate(self.rng.shuffled(PLANE_FEATURES)):
            if k == 2:
                self.init(self.s.size)                   # (a fresh replay stays short)
                self.render(passes=1)
            self.observe(self._entry(f), pass_begin=self.rng.pick([b for b in PLANE_PASSES[f] if b != self.s.next_pass]))
            self.render(passes=1)
        self.observe("read_accum")

    def motif_device_then_host(self):
        """the device entry (on the side stream in a side-stream schedule) directly followed by the host entry of the same feature: the
        fence and the stream it was recorded on"""
        self.init()
        self.render(passes=1)
        for f in self.rng.shuffled(PLANE_FEATURES):
            self.observe(f + "_device")
            self.observe(f)
        self.observe("render_readback", passes=1)

    def motif_group_table_change(self):
        """another table after the scene changed, at an unchanged frame size: what was uploaded last"""
        self.init()
        self.render(passes=1)
        first = self.rng.pick(GROUP_TABLES)
        self.observe(self._entry("light_groups"), table=first)
        self.mutate("update_scene" if FAMILIES[self.family]["update"] else "refit_mesh")          # (and an init at the same size)
        self.observe(self._entry("light_groups"), table=self.rng.pick([t for t in GROUP_TABLES if t != first]))
        self.observe(self._entry("light_groups"), table=first)
        self.observe("render_readback", passes=1)

    def motif_bake_neutral(self):
        """a baked instance across operations that leave the logical state: the installed code object and its key"""
        self.init()
        self.emit("set_bake", mode=1, share=0)
        self.emit("reserve", passes=2, depth=4)          # (with mode 1 this is where the instance is compiled and installed)
        self.render(depth=4, passes=1)
        self.emit("rebuild_there_and_back")
        self.render(depth=4, passes=1)
        self.emit("fast_there_and_back")
        self.observe("render_readback", depth=4, passes=1)
        self.emit("set_tuning", fields=dict(self.rng.pick(TUNINGS)))                               # drops the mode
        self.observe("render_readback", depth=4, passes=1)
        self.emit("set_bake", mode=1, share=0)           # and back on: what the golden anchor may find in force

    def motif_scene_sweep(self):
        """the scene changes, then every observer kind looks"""
        self.init()
        self.render(passes=1)
        self.mutate("update_scene" if FAMILIES[self.family]["update"] else "refit_mesh")
        self.init(self.rng.pick(SIZES[1:4]))
        self.render(passes=2)
        for kind in self.rng.shuffled(OBSERVERS):
            self.observe(kind)

    def anchor(self):
        """the end of every schedule on a scene with a golden file: the file's own frame on the live renderer, after its whole history"""
        g = FAMILIES[self.family]["golden"]
        if not g:
            return
        W, H, depth, passes = GOLDEN_FRAMES[g]
        self.reserve = 0
        if self.s.scene[0] == "refit":
            self.emit("refit_mesh", amount=REFITS[2][0], normals=REFITS[2][1])
        if self.s.shard != DEFAULT_SHARD:
            self.emit("set_shard", rank=0, world=1, tile=32)
        if self.s.roulette:
            self.emit("set_russian_roulette", start=0)
        if self.s.probe:
            self.emit("set_probe_sampling", mode=0)
        if self.small_batches:                           # (the per-path radiance is read from ONE batch)
            self.emit("set_batch_paths", paths=8 << 20)
        if self.lookahead:                               # (and would be seen one call ahead)
            self.emit("set_lookahead", mode=0)
        self.emit("init", size=(W, H))
        self.emit("set_pass_index", index=0)
        self.emit("render_readback", depth=depth, mode="pathtrace", passes=passes, golden=True)


MOTIFS = ("shrink_grow", "depth_and_pipeline", "shared_buffers", "seed_table", "shard", "lookahead", "planes_shrink_grow",
          "planes_between_renders", "device_then_host", "group_table_change", "bake_neutral", "scene_sweep")
ANYWHERE = MOTIFS[:9]                             # the motifs every scene family supports
MOTIF_OPS = {"planes_shrink_grow": 20, "planes_between_renders": 14}             # the ops a motif takes where that is more than 14


def schedule(seed):
    """The schedule of a seed: pure and deterministic.  A motif or two (the sequences that caches are most likely to get wrong), then a random
    walk over mutators, live-only settings, there-and-back operations, refused calls and observers, then the golden anchor."""
    b = _Builder(seed)
    r = b.rng
    scene_changes = FAMILIES[b.family]["update"] or FAMILIES[b.family]["refit"]
    first = MOTIFS[(seed//len(FAMILY_ORDER)) % len(MOTIFS)]
    if (first in ("scene_sweep", "group_table_change") and not scene_changes) or (first == "bake_neutral" and b.family != "cornell"):
        first = r.pick(ANYWHERE)
    getattr(b, "motif_" + first)()
    if first != "scene_sweep" and r.below(2):
        second = r.pick([m for m in ANYWHERE if m != first])
        if b.room() >= MOTIF_OPS.get(second, 14):
            getattr(b, "motif_" + second)()
    mutators = [k for k in MUTATORS if supports(b.family, k)]
    rare = [k for k in ("set_probe_sampling", "refit_mesh", "update_scene") if supports(b.family, k)]
    lookers = r.shuffled(OBSERVERS)              # every observer kind in turn, so that none is left out of the second half
    walk = b.room()
    while b.room() > 0:
        before = len(b.ops)
        early = 3*(walk - b.room()) < walk       # settings and mutators first, observers behind them
        x = r.below(100)
        if rare and early and x < 15:
            b.mutate(rare[0])
        elif x < (45 if early else 8):
            b.mutate(r.pick(mutators))
        elif x < (80 if early else 14):
            b.live_only(r.pick(LIVE_ONLY))
        elif x < (86 if early else 20):
            b.neutral(r.pick(THERE_AND_BACK))
        elif x < (92 if early else 26):
            b.neutral(r.pick(REFUSED))
        else:
            b.observe(lookers.pop())
            lookers = lookers or r.shuffled(OBSERVERS)
        if b.room() < 0:                                  # (an op that brought an init with it and no longer fits)
            del b.ops[before:]
            b = _rebuilt(b, seed)
            break
    b.anchor()
    assert len(b.ops) <= MAX_OPS, len(b.ops)
    return b.ops


def _rebuilt(b, seed):
    """a builder brought to the truncated op list (the model replayed from the start)"""
    ops = b.ops
    n = _Builder(seed)
    n.ops, n.model = [], Model()
    for op in ops:
        n.emit(op[0], **op[1])
    return n


# -- what a schedule covers (tests/test_renderer_model.py) ------------------------------------------------------------------------------------

def observations(ops):
    return [k for k, op in enumerate(ops) if op[0] in OBSERVERS]


def shrinks_and_grows(ops):
    areas = [p["size"][0]*p["size"][1] for k, p in ops if k in INITS]
    return any(a > b for a, b in zip(areas, areas[1:])) and any(a < b for a, b in zip(areas, areas[1:]))


def pairs(ops, firsts):
    """the (first kind, observer kind) pairs of a schedule in which the first kind precedes the observer"""
    seen, out = set(), set()
    for kind, _ in ops:
        if kind in OBSERVERS:
            out.update((m, kind) for m in seen)
        # (render_readback is a render too, but it is counted as the observer it is)
        if kind in firsts:
            seen.add(kind)
    return out


def _renders(ops):
    """(step, op, first pass) of every path-traced render, and the steps of the ops between them, from the model's point of view"""
    m, out = Model(), []
    for k, op in enumerate(ops):
        before = m.state.next_pass if m.state else 0
        m.apply(k, op)
        if op[0] in ("render", "render_async", "render_readback") and op[1]["mode"] == "pathtrace":
            out.append((k, op, before))
    return out


def _between(ops, a, b, kinds):
    return [k for k in range(a + 1, b) if ops[k][0] in kinds]


INITS = ("init", "init_external")


def sequences(ops):
    """the names of the required sequences (tests/test_renderer_model.py) a schedule holds"""
    found = set()
    kinds = [k for k, _ in ops]
    rs = _renders(ops)
    # shrink then grow, present with NLM and denoise at each of the three sizes
    frames = []
    for k, (kind, p) in enumerate(ops):
        if kind in INITS:
            frames.append([p["size"][0]*p["size"][1], False, False])
        elif frames and kind == "present" and p["nlm"] > 0:
            frames[-1][1] = True
        elif frames and kind == "denoise_own":
            frames[-1][2] = True
    full = [f[0] for f in frames if f[1] and f[2]]
    if any(full[i] > full[i + 1] < full[i + 2] for i in range(len(full) - 2)):
        found.add("shrink_grow")
    for (a, oa, _), (b, ob, _), (c, oc, _) in zip(rs, rs[1:], rs[2:]):
        if oa[1]["depth"] > ob[1]["depth"] < oc[1]["depth"] and not _between(ops, a, c, ("set_pipeline", "set_tuning", "set_shard") + INITS):
            found.add("depth_down_up")
    for (a, oa, pa), (b, ob, _) in zip(rs, rs[1:]):
        mid = lambda ks: _between(ops, a, b, ks)                                                      # noqa: E731
        if mid(("set_pipeline",)) and not mid(INITS + ("set_tuning", "set_shard")):
            found.add("pipeline_change_allocated")
        if mid(("radiance", "gather", "gather_sh")) and not mid(INITS):
            found.add("query_between_renders")
        for k in mid(("features", "features_device", "id_mattes", "id_mattes_device")):
            # (its own pass_begin: not the pass the renderer is at)
            if ops[k][1]["pass_begin"] != pa + oa[1]["passes"] and not mid(INITS + ("set_pass_index",)):
                found.add("side_pass_between_renders")
        if mid(("set_shard",)) and not mid(INITS):
            found.add("shard_change_same_frame")
    for i, (a, oa, pa) in enumerate(rs):
        for j in range(i + 1, len(rs)):
            if rs[j][2] >= pa + SEED_TABLE_AHEAD + 1 and any(r[2] < rs[j][2] for r in rs[j + 1:]):
                found.add("seed_table_exit_and_rewind")
    on = 0
    last = None         # (step, depth, passes) of the last read-back render with look-ahead on: it speculates on a repeat
    for k, (kind, p) in enumerate(ops):
        if kind == "set_lookahead":
            on, last = p["mode"], None
        elif kind == "render_readback" and on:
            if last is not None and (p["depth"], p["passes"]) != last[1:] and not _between(ops, last[0], k, ALL_KINDS):
                found.add("lookahead_miss")
            if last is not None and [ops[x][0] for x in range(last[0] + 1, k)] == ["present"]:
                found.add("lookahead_across_present")
            last = (k, p["depth"], p["passes"]) if p["mode"] == "pathtrace" else None
        elif kind != "present":
            last = None
    for m in ("update_scene", "refit_mesh"):
        if m in kinds and set(OBSERVERS) <= set(kinds[kinds.index(m) + 1:]):
            found.add(m + "_then_every_observer")
    found |= _plane_sequences(ops, rs)
    return found


def _planes_per_pixel(kind, p):
    """what a plane call keeps per pixel of the frame, roughly: paths times planes (a sample map: its mean count)"""
    f = feature_of(kind)
    if f == "sample_map":
        return {"zeros": 0.0, "crop": 0.25, "random": 1.5, "uniform": 2.0}[p["map"]]
    return p["passes"]*{"light_groups": lambda: group_table(p["table"], 0)[2], "views": lambda: p["count"], "depth_planes": lambda: len(p["depths"])}[f]()


def _plane_sequences(ops, rs):
    """the sequences of the plane features (light groups, views, sample maps, depth planes) and of the bake mode"""
    found = set()
    # every feature at three successive frames, big, smaller, bigger again, with a render before the first look and after the last
    frames = []                                          # [area, {feature: (first step, last step, paths of the largest call)}] per init
    for k, (kind, p) in enumerate(ops):
        if kind in INITS:
            frames.append([p["size"][0]*p["size"][1], {}])
        elif frames and feature_of(kind):
            first, _, paths = frames[-1][1].get(feature_of(kind), (k, k, 0))
            frames[-1][1][feature_of(kind)] = (first, k, max(paths, frames[-1][0]*_planes_per_pixel(kind, p)))
    steps = [r[0] for r in rs]

    def shrinks_then_grows(f):
        # (and the last of the three asks for more than the first: buffers that kept their first size would be too small for it)
        for a, b, c in zip(frames, frames[1:], frames[2:]):
            if f in a[1] and f in b[1] and f in c[1] and a[0] > b[0] < c[0] and steps and min(steps) < a[1][f][0] and max(steps) > c[1][f][1] \
                    and a[1][f][2] > b[1][f][2] < c[1][f][2] > a[1][f][2]:
                return True
        return False
    if all(shrinks_then_grows(f) for f in PLANE_FEATURES):
        found.add("planes_shrink_grow")
    # a plane call at a pass of its own between two renders of one frame
    for (a, oa, pa), (b, ob, _) in zip(rs, rs[1:]):
        if _between(ops, a, b, INITS + ("set_pass_index",)):
            continue
        for k in _between(ops, a, b, PLANE_OBSERVERS):
            if ops[k][1]["pass_begin"] != pa + oa[1]["passes"]:
                found.add(feature_of(ops[k][0]) + "_between_renders")
    # the device entry on a side stream, then at once the host entry of the same feature
    for (ka, pa), (kb, _) in zip(ops, ops[1:]):
        if ka.endswith("_device") and feature_of(ka) == kb and pa.get("stream"):
            found.add(kb + "_device_then_host")
    # two light-group tables, the second after the scene changed, no other frame size between them
    last, changed, size = None, False, None
    for kind, p in ops:
        if kind in INITS:
            if tuple(p["size"]) != size:
                last = None
            size = tuple(p["size"])
        elif kind in ("update_scene", "refit_mesh"):
            changed = last is not None
        elif feature_of(kind) == "light_groups":
            if last is not None and changed and p["table"] != last:
                found.add("group_table_change")
            last, changed = p["table"], False
    # the bake mode across operations that leave the logical state, on the scene whose plan gives the closed fused kernel
    if ops[0][1]["scene"] == "cornell":
        want = [lambda k, p: k == "set_bake" and (p["mode"], p["share"]) == (1, 0), lambda k, p: k in ("render", "render_async"),
                lambda k, p: k == "rebuild_there_and_back", lambda k, p: k in ("render", "render_async"),
                lambda k, p: k == "fast_there_and_back", lambda k, p: k == "render_readback", lambda k, p: k == "set_tuning",
                lambda k, p: k == "render_readback"]
        for start in range(len(ops)):
            at = 0
            for kind, p in ops[start:]:
                if want[at](kind, p):
                    at += 1
                    if at == len(want):
                        break
                elif at and kind not in INITS + ("reserve",):
                    break
            if at == len(want):
                found.add("bake_across_neutral_ops")
        force = None
        for kind, p in ops:
            if kind in ("set_tuning", "set_bake"):
                force = (p["mode"], p["share"]) if kind == "set_bake" else None
        if force == (1, 0) and ops[-1][1].get("golden"):
            found.add("bake_in_force_at_the_anchor")
    return found


SEQUENCES = ("shrink_grow", "depth_down_up", "pipeline_change_allocated", "query_between_renders", "side_pass_between_renders",
             "seed_table_exit_and_rewind", "shard_change_same_frame", "lookahead_miss", "lookahead_across_present",
             "update_scene_then_every_observer", "refit_mesh_then_every_observer", "planes_shrink_grow", "group_table_change",
             "bake_across_neutral_ops", "bake_in_force_at_the_anchor") + \
    tuple(f + s for f in PLANE_FEATURES for s in ("_between_renders", "_device_then_host"))


# parameter values the schedules must draw somewhere: (kind prefix, parameter, value)
VALUES = tuple([("render", "mode", m) for m in ("pathtrace", "normals")] + [("render", "passes", n) for n in (1, 2, 3)] +
               [("init", "size", z) for z in SIZES] + [("refit_mesh", "normals", n) for n in (None, 7)] +
               [("id_mattes", "slots", n) for n in (1, 4, 8)] + [("features", "mask", n) for n in range(1, 8)] +
               [("present", "nlm", n) for n in (0, 1, 2)] + [("gather_sh", "order", n) for n in (0, 1, 2)] +
               [("gather", "mode", m) for m in ("cosine", "sphere")] + [("trace_rays", "mode", m) for m in ("closest", "occluded")] +
               [("set_batch_paths", "paths", 1024), ("set_counters", "timing", True), ("set_counters", "detail", True),
                ("denoise_own", "guides", True), ("denoise_own", "guides", False)] +
               [(k, "device", d) for k in ("radiance", "gather", "gather_sh", "denoise_own", "denoise_images") for d in (False, True)] +
               [(f, "pass_begin", b) for f in PLANE_FEATURES for b in PLANE_PASSES[f]] +
               [(f, "passes", n) for f in ("light_groups", "views", "depth_planes") for n in (1, 2)] +
               [(f, name, x) for f in ("views", "depth_planes") for name in ("add", "singly") for x in (False, True)] +
               [("sample_map", "add", x) for x in (False, True)] + [("light_groups", "table", t) for t in GROUP_TABLES] +
               [("views", "count", n) for n in VIEW_COUNTS] + [("sample_map", "map", m) for m in SAMPLE_MAPS] +
               [("depth_planes", "depths", d) for d in PLANE_DEPTHS] +
               [("refused_planes", "feature", f) for f in PLANE_FEATURES] + [("refused_planes", "device", d) for d in (False, True)] +
               [("set_bake", "mode", m) for m in BAKE_MODES] + [("set_bake", "share", n) for n in BAKE_SHARES])


def requirements():
    """token -> in how many schedules it must occur"""
    need = {("kind", k): 2 for k in ALL_KINDS if k != "create"}
    need.update({("pair", m, o): 1 for m in MUTATORS for o in OBSERVERS})
    need.update({("pair", s, o): 1 for s in LIVE_ONLY for o in OBSERVERS})
    need.update({("sequence", s): 1 for s in SEQUENCES})
    need.update({("tuning", f): 1 for f in TUNING_FIELDS})
    need.update({("pipeline", p): 1 for p in PIPELINES})
    need.update({("lookahead", m): 1 for m in (0, 1, 2)})
    need.update({("family", f): 1 for f in FAMILY_ORDER})
    need.update({("value",) + v: 1 for v in VALUES})
    need[("side_stream",)] = 3
    return need


def tokens(ops):
    out = {("kind", k) for k, _ in ops}
    out.add(("family", ops[0][1]["scene"]))
    out.update(("pair",) + p for p in pairs(ops, MUTATORS + LIVE_ONLY))
    out.update(("sequence", s) for s in sequences(ops))
    for prefix, name, value in VALUES:
        if any(kind.startswith(prefix) and name in p and p[name] == value for kind, p in ops):
            out.add(("value", prefix, name, value))
    for kind, p in ops:
        if kind == "set_tuning":
            out.update(("tuning", f) for f in p["fields"] if f in TUNING_FIELDS)
        if kind == "set_bake":
            out.update((("tuning", "bounce_share"), ("tuning", "bounce_bake")))
        if kind == "set_pipeline":
            out.add(("pipeline", p["pipeline"]))
        if kind == "set_lookahead":
            out.add(("lookahead", p["mode"]))
        if p.get("stream"):
            out.add(("side_stream",))
    return out


def choose_seeds(candidates=range(600), limit=MAX_SCHEDULES):
    """How SEEDS was chosen: greedily, the candidate whose schedule meets most of what is still missing, until nothing is (a schedule with
    fewer than 10 observations is no candidate).  Returns (seeds, what is still missing)."""
    need = requirements()
    have = {}
    for s in candidates:
        ops = schedule(s)
        if len(observations(ops)) >= 10 and shrinks_and_grows(ops):
            have[s] = tokens(ops) & set(need)
    chosen = []
    for again in (False, True):
        if again:                                        # what is left of the 16: the sequences and the scenes a second time
            need.update({t: 1 for t in need if t[0] in ("sequence", "family")})
        _greedy(need, have, chosen, limit)
    return sorted(chosen), {t: n for t, n in requirements().items() if sum(t in have[s] for s in chosen) < n}


def _greedy(need, have, chosen, limit):
    while any(need.values()) and len(chosen) < limit:
        best = max((s for s in have if s not in chosen), key=lambda s: (sum(1 for t in have[s] if need[t] > 0), -s))
        if not any(need[t] > 0 for t in have[best]):
            break
        chosen.append(best)
        for t in have[best]:
            need[t] = max(0, need[t] - 1)


# choose_seeds(range(3000)): what meets requirements(), topped up to 16 with seeds that repeat sequences on other scenes
SEEDS = (3, 54, 65, 234, 392, 426, 715, 936, 1328, 1370, 1614, 1902, 2239, 2506, 2529, 2657)
# The set chosen before the plane features and the bake mode joined the model (MAX_OPS 32).  The schedules these seeds give under the present
# generator are run as well -- further histories that no requirement selected, each with at least 10 observations -- but nothing in
# requirements() counts on them: what must be covered is covered by SEEDS alone.
EARLIER_SEEDS = (33, 37, 44, 322, 540, 725, 908, 948, 955, 1374, 1614, 1644, 1662, 1976, 2337, 2762)
ALL_SEEDS = SEEDS + tuple(s for s in EARLIER_SEEDS if s not in SEEDS)


# -- groups -------------------------------------------------------------------------------------------------------------------------------------

GROUPS = ((2, 32, "features_probe", 101), (3, 16, "cornell", 202))       # (members, tile, scene, seed)


def group_schedule(seed):
    """ops of a HipRendererGroup: init at changing sizes, option and depth changes, look-ahead modes; render with and without read-back and
    present observe.  The model is the same State: a group has no shard, roulette or probe setting of its own."""
    r = _Rng(seed)
    ops, renders, mode = [], 0, 0
    sizes = r.shuffled(SIZES)
    for size in sizes[:4]:
        ops.append(("init", {"size": size}))
        renders = 0
        for _ in range(5):
            x = r.below(10)
            if x < 2:
                mode = r.pick([m for m in (0, 1, 2) if m != mode])
                ops.append(("set_lookahead", {"mode": mode}))
            elif x < 4 and renders:
                ops.append(("present", {"nlm": r.below(3)}))
            elif renders < MAX_REPLAY_RENDERS:
                kind = "render" if x == 4 else "render_readback"
                ops.append((kind, {"depth": r.pick(DEPTHS[:3]), "mode": "normals" if x == 9 else "pathtrace", "passes": 1 + r.below(2)}))
                renders += 1
    return ops[:MAX_OPS]

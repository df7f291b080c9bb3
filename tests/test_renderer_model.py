"""The committed schedules of tests/renderer_model.py, judged without a GPU: what they cover is a condition on SEEDS, so that a thin set of
histories cannot pass for a thorough one.  tests/test_gpu_histories.py runs the same schedules on a live renderer."""
import os

import numpy as np
import pytest

from tests import renderer_model as rm

SCHEDULES = {seed: rm.schedule(seed) for seed in rm.SEEDS}
# (with the earlier set's seeds, which are run too: what a schedule must be on its own is asked of them as well, what the SET must cover of
# SCHEDULES alone)
ALL = {seed: SCHEDULES[seed] if seed in SCHEDULES else rm.schedule(seed) for seed in rm.ALL_SEEDS}


def test_the_set_is_small():
    assert 0 < len(rm.SEEDS) <= rm.MAX_SCHEDULES and len(set(rm.SEEDS)) == len(rm.SEEDS)
    for seed, ops in SCHEDULES.items():
        assert len(ops) <= rm.MAX_OPS, seed
        assert ops[0][0] == "create" and all(k != "create" for k, _ in ops[1:]), seed


@pytest.mark.parametrize("seed", rm.ALL_SEEDS)
def test_schedule_is_reproducible_and_a_literal(seed):
    again = rm.schedule(seed)
    assert again == ALL[seed] and again is not ALL[seed]
    assert eval(repr(again), {}) == again                    # what a failure message prints replays as it is


@pytest.mark.parametrize("seed", rm.ALL_SEEDS)
def test_schedule_observes_at_least_ten_times(seed):
    assert len(rm.observations(ALL[seed])) >= 10


@pytest.mark.parametrize("seed", rm.ALL_SEEDS)
def test_schedule_is_valid_for_its_scene_and_its_replays_stay_short(seed):
    """every op is one the scene supports (Model.apply asserts it), and at every step a fresh renderer gets there with at most 4 render
    calls and 8 passes"""
    m = rm.Model()
    for k, op in enumerate(ALL[seed]):
        m.apply(k, op)
        if any(r[0] != m.state.scene for r in m.state.renders):      # the scene changed under a frame: nothing looks before the next init
            assert ALL[seed][k + 1][0] in ("init", "init_external", "set_shard", "set_russian_roulette", "set_batch_paths", "set_lookahead"), (seed, k)
            continue
        renders = [s for s in rm.replay(m.state) if s[0] == "render"]
        assert len(renders) <= rm.MAX_REPLAY_RENDERS and sum(s[3] for s in renders if s[2] == "pathtrace") <= rm.MAX_REPLAY_PASSES, (seed, k)
        assert not m.state.dirty and m.state.arith == 0


def test_every_op_kind_occurs_in_two_schedules():
    for kind in rm.ALL_KINDS[1:]:
        n = sum(any(k == kind for k, _ in ops) for ops in SCHEDULES.values())
        assert n >= 2, "%s occurs in %d schedules" % (kind, n)


def _table(firsts):
    covered = {}
    for seed, ops in SCHEDULES.items():
        for pair in rm.pairs(ops, firsts):
            covered.setdefault(pair, []).append(seed)
    width = max(len(f) for f in firsts)
    print("\n%s  %s" % (" "*width, " ".join("%2d" % k for k in range(len(rm.OBSERVERS)))))
    for f in firsts:
        print("%-*s  %s" % (width, f, " ".join("%2d" % len(covered.get((f, o), ())) for o in rm.OBSERVERS)))
    print("columns: " + ", ".join("%d %s" % (k, o) for k, o in enumerate(rm.OBSERVERS)) + "; entries: schedules in which the row precedes the column")
    return covered


def test_every_mutator_precedes_every_observer_somewhere():
    covered = _table(rm.MUTATORS)
    wanted = [(m, o) for m in rm.MUTATORS for o in rm.OBSERVERS if any(rm.supports(f, m) for f in rm.FAMILIES)]
    assert len(wanted) == len(rm.MUTATORS)*len(rm.OBSERVERS)             # every mutator has a scene that supports it
    print("%d (mutator, observer) pairs wanted, %d exercised" % (len(wanted), len(covered)))
    assert not [p for p in wanted if p not in covered]


def test_every_live_only_setting_precedes_every_observer_somewhere():
    covered = _table(rm.LIVE_ONLY)
    assert not [(s, o) for s in rm.LIVE_ONLY for o in rm.OBSERVERS if (s, o) not in covered]
    seen = set().union(*(rm.tokens(ops) for ops in SCHEDULES.values()))
    assert not [f for f in rm.TUNING_FIELDS if ("tuning", f) not in seen]
    assert not [p for p in rm.PIPELINES if ("pipeline", p) not in seen]
    assert not [m for m in (0, 1, 2) if ("lookahead", m) not in seen]
    assert any(op == ("set_batch_paths", {"paths": 1024}) for ops in SCHEDULES.values() for op in ops)
    assert any(k == "set_counters" and p["timing"] for ops in SCHEDULES.values() for k, p in ops)
    assert any(k == "set_counters" and p["detail"] for ops in SCHEDULES.values() for k, p in ops)


@pytest.mark.parametrize("name", rm.SEQUENCES)
def test_sequence_is_present(name):
    assert [seed for seed, ops in SCHEDULES.items() if name in rm.sequences(ops)], name


def test_the_whole_requirement_table_holds_on_the_committed_seeds():
    have = [rm.tokens(ops) for ops in SCHEDULES.values()]
    short = {t: n for t, n in rm.requirements().items() if sum(t in h for h in have) < n}
    assert not short, short


def test_the_committed_seeds_are_what_choose_seeds_returns():
    seeds, missing = rm.choose_seeds(range(3000))
    assert not missing, missing
    assert tuple(seeds) == rm.SEEDS


def test_mutators_draw_what_the_issue_lists():
    ops = [op for s in SCHEDULES.values() for op in s]
    sizes = {p["size"] for k, p in ops if k in ("init", "init_external")}
    assert set(rm.SIZES) <= sizes
    for seed, s in SCHEDULES.items():
        areas = [p["size"][0]*p["size"][1] for k, p in s if k in ("init", "init_external")]
        assert any(a > b for a, b in zip(areas, areas[1:])) and any(a < b for a, b in zip(areas, areas[1:])), "%d: shrink and grow" % seed
    renders = [p for k, p in ops if k in ("render", "render_async", "render_readback")]
    assert {p["mode"] for p in renders} == {"pathtrace", "normals"} and {1, 2, 3} <= {p["passes"] for p in renders}
    assert any(k == "refit_mesh" and p["normals"] is None for k, p in ops) and any(k == "refit_mesh" and p["normals"] for k, p in ops)
    assert {p["slots"] for k, p in ops if k.startswith("id_mattes")} == {1, 4, 8}
    assert {p["mask"] for k, p in ops if k.startswith("features")} == set(range(1, 8))
    assert {p["nlm"] for k, p in ops if k == "present"} == {0, 1, 2}
    assert {p["order"] for k, p in ops if k == "gather_sh"} == {0, 1, 2}
    assert {p["mode"] for k, p in ops if k == "gather"} == {"cosine", "sphere"}
    assert {p["mode"] for k, p in ops if k.startswith("trace_rays")} == {"closest", "occluded"}
    # device entries on a non-default stream in at least three schedules, and the op behind one is a host entry on the default stream
    assert sum(any(p.get("stream") for _, p in s) for s in SCHEDULES.values()) >= 3
    host_next = lambda s: any(a[1].get("stream") and not ("stream" in b[1]) for a, b in zip(s, s[1:]))           # noqa: E731
    assert sum(host_next(s) for s in SCHEDULES.values()) >= 3
    assert {s[0][1]["scene"] for s in SCHEDULES.values()} == set(rm.FAMILIES)


def test_plane_observers_draw_what_the_issue_lists():
    """light groups, views, sample maps and depth planes, host and device entry: every listed value somewhere, frames the model's SIZES,
    passes and counts 1 to 3, and never a sharded renderer in front of one"""
    ops = [op for s in SCHEDULES.values() for op in s]
    of = lambda f: [p for k, p in ops if rm.feature_of(k) == f]                                                  # noqa: E731
    for kind in rm.PLANE_OBSERVERS:
        assert kind in rm.FRAME_OBSERVERS and rm.replay_level(kind) == "frame"
        assert sum(any(k == kind for k, _ in s) for s in SCHEDULES.values()) >= 2, kind
    for f in rm.PLANE_FEATURES:
        assert {p["pass_begin"] for p in of(f)} == set(rm.PLANE_PASSES[f]), f
        assert all(("stream" in p) == k.endswith("_device") for k, p in ops if rm.feature_of(k) == f), f
    for f in ("light_groups", "views", "depth_planes"):
        assert {p["passes"] for p in of(f)} == {1, 2}, f
    for f in ("views", "depth_planes"):
        assert {(p["add"], p["singly"]) for p in of(f)} == {(a, s) for a in (False, True) for s in (False, True)}, f
    assert {p["add"] for p in of("sample_map")} == {False, True}
    assert {p["table"] for p in of("light_groups")} == set(rm.GROUP_TABLES) == {"one", "parity", "eight"}
    assert {p["count"] for p in of("views")} == set(rm.VIEW_COUNTS) == {1, 3, 6}
    assert {p["map"] for p in of("sample_map")} == set(rm.SAMPLE_MAPS) == {"uniform", "random", "crop", "zeros"}
    assert {p["depths"] for p in of("depth_planes")} == set(rm.PLANE_DEPTHS) == {(1,), (1, 2, 3, 4), (2, 6), tuple(range(1, 17))}
    assert all(p["seed"] in (1, 2, 3) for f in rm.PLANE_FEATURES[1:] for p in of(f))
    for seed, s in SCHEDULES.items():
        m = rm.Model()
        for k, op in enumerate(s):
            if op[0] in rm.PLANE_OBSERVERS:
                assert m.state.shard[1] == 1 and m.state.arith == 0 and m.state.size in rm.SIZES, (seed, k)
            m.apply(k, op)
    # the refused calls: each feature, host and device entry
    refused = [p for k, p in ops if k in ("refused_planes_sharded", "refused_planes_fast")]
    assert {p["feature"] for p in refused} == set(rm.PLANE_FEATURES) and {p["device"] for p in refused} == {False, True}
    assert set(rm.REFUSED_PLANES) == set(rm.PLANE_FEATURES)


def test_group_tables_are_made_from_the_primitive_count_alone():
    assert rm.group_table("one", 9) == ([0]*9, 0, 1)
    assert rm.group_table("parity", 5) == ([0, 1, 0, 1, 0], 1, 2)
    table, env, groups = rm.group_table("eight", 16)
    assert (env, groups) == (-1, 8) and table == [0, 1, 2, 3, 4, 5, -1, 7, 0, 1, 2, 3, 4, -1, 6, 7]
    assert rm.group_table("eight", 3) == ([0, 1, 2], -1, 8)              # G stays 8 where the scene has fewer primitives


def test_the_bake_mode_is_live_only_and_a_set_tuning_drops_it():
    assert "set_bake" in rm.LIVE_ONLY and {"bounce_share", "bounce_bake"} <= set(rm.TUNING_FIELDS)
    ops = [op for s in SCHEDULES.values() for op in s]
    assert {(p["mode"], p["share"]) for k, p in ops if k == "set_bake"} >= {(1, 0)}
    assert {p["mode"] for k, p in ops if k == "set_bake"} == {1, 0, -1} and {p["share"] for k, p in ops if k == "set_bake"} == {0, -1}
    m = rm.Model()
    for k, op in enumerate([("create", {"scene": "cornell"}), ("init", {"size": (16, 16)}), ("set_bake", {"mode": 1, "share": 0})]):
        m.apply(k, op)
    assert rm.replay(m.state) == [("create", ("pack", "cornell")), ("init", 16, 16)]          # the fresh renderer never gets it
    # the builder knows what is in force: a set_tuning drops the mode (and the small batches), as the library does
    b = rm._Builder(5)
    b.emit("set_batch_paths", paths=1024)
    b.emit("set_bake", mode=1, share=0)
    assert b.bake == (1, 0) and not b.small_batches
    b.emit("set_tuning", fields={})
    assert b.bake is None
    # on cornell: the mode across a rebuild, the tolerance arm and a set_tuning; and a schedule whose golden anchor finds the mode in force
    for name in ("bake_across_neutral_ops", "bake_in_force_at_the_anchor"):
        assert [s for s, o in SCHEDULES.items() if name in rm.sequences(o) and o[0][1]["scene"] == "cornell"], name


def test_the_teeth_bite_at_an_observation_of_the_kind_they_name():
    from tests import test_gpu_histories as th
    kinds = {}
    for what, (ops, forget, expected) in th.TEETH.items():
        m = rm.Model()
        for k, op in enumerate(ops):
            m.apply(k, op)                                               # a valid schedule
        assert [k for k in rm.observations(ops) if k > forget[0]][0] == expected, what
        kinds[rm.feature_of(ops[expected][0])] = ops[0][1]["scene"], ops[forget[0]][0]
    assert all(kinds.get(f) == ("anim_cornell", "update_scene") for f in rm.PLANE_FEATURES), kinds
    m = rm.Model()
    for k, op in enumerate(th.BAKED):
        m.apply(k, op)
    assert th.BAKED[:3] == [("create", {"scene": "cornell"}), ("set_bake", {"mode": 1, "share": 0}), ("init", {"size": (64, 64)})]
    assert th.BAKED[-1][1].get("golden") and rm.GOLDEN_FRAMES["cornell"] == (64, 64, 4, 4)


def test_every_schedule_on_a_scene_with_a_golden_file_ends_on_it(golden_dir):
    from tinsel_amd import abi
    for seed, ops in SCHEDULES.items():
        name = rm.FAMILIES[ops[0][1]["scene"]]["golden"]
        if not name:
            continue
        g = np.load(os.path.join(golden_dir, name + ".golden.npz"))
        opt = abi.Options.from_buffer_copy(g["options"].tobytes())
        assert rm.GOLDEN_FRAMES[name] == (opt.width, opt.height, opt.max_depth, int(g["passes"]))
        W, H, depth, passes = rm.GOLDEN_FRAMES[name]
        assert ops[-3:] == [("init", {"size": (W, H)}), ("set_pass_index", {"index": 0}),
                            ("render_readback", {"depth": depth, "mode": "pathtrace", "passes": passes, "golden": True})], seed
        m = rm.Model()
        for k, op in enumerate(ops):
            m.apply(k, op)
        s = m.state
        assert (s.shard, s.roulette, s.probe) == (rm.DEFAULT_SHARD, 0, 0), seed
        assert s.scene == ("pack", name) or s.scene == ("refit", name) + rm.REFITS[2], seed


def test_replay_is_minimal_and_launches_nothing():
    m = rm.Model()
    ops = [("create", {"scene": "features_probe"}), ("set_russian_roulette", {"start": 2}), ("init", {"size": (96, 64)}),
           ("render", {"depth": 4, "mode": "pathtrace", "passes": 2}), ("set_pipeline", {"pipeline": "split"}),
           ("init", {"size": (33, 17)}), ("set_pass_index", {"index": 1030}), ("render", {"depth": 3, "mode": "pathtrace", "passes": 1}),
           ("set_shard", {"rank": 1, "world": 2, "tile": 16}), ("set_probe_sampling", {"mode": 1}),
           ("render_readback", {"depth": 2, "mode": "pathtrace", "passes": 2}), ("set_pass_index", {"index": 4}),
           ("features", {"mask": 7, "pass_begin": 0, "passes": 1})]
    for k, op in enumerate(ops):
        m.apply(k, op)
    assert rm.replay(m.state) == [
        ("create", ("pack", "features_probe")), ("set_russian_roulette", 2), ("init", 33, 17), ("set_pass_index", 1030),
        ("render", 3, "pathtrace", 1), ("set_shard", 1, 2, 16), ("set_probe_sampling", 1), ("render", 2, "pathtrace", 2),
        ("set_pass_index", 4)]
    assert rm.replay(m.state, "scene") == [("create", ("pack", "features_probe")), ("set_shard", 1, 2, 16), ("set_russian_roulette", 2),
                                           ("set_probe_sampling", 1)]
    assert rm.replay(m.state, "frame") == rm.replay(m.state, "scene") + [("init", 33, 17), ("set_pass_index", 4)]
    m.apply(len(ops), ("write_accum", {"seed": 2, "next_pass": 9}))
    assert rm.replay(m.state)[-2:] == [("init", 33, 17), ("write_accum", 2, 9)]


def test_a_sabotaged_model_believes_something_else():
    ops = [("create", {"scene": "cornell"}), ("init", {"size": (48, 32)}), ("set_pass_index", {"index": 5}), ("init", {"size": (16, 16)})]
    states = []
    for forget in (None, (2, "op"), (3, "size")):
        m = rm.Model(forget)
        for k, op in enumerate(ops):
            m.apply(k, op)
        states.append((m.state.size, m.state.next_pass))
    assert states == [((16, 16), 5), ((16, 16), 0), ((48, 32), 5)]


def test_group_schedules_are_reproducible_and_observe():
    for n, tile, scene, seed in rm.GROUPS:
        ops = rm.group_schedule(seed)
        assert ops == rm.group_schedule(seed) and len(ops) <= rm.MAX_OPS
        kinds = [k for k, _ in ops]
        assert sum(k in ("render_readback", "present") for k in kinds) >= 8
        assert {"init", "set_lookahead", "render_readback", "present", "render"} <= set(kinds), kinds
        sizes = [p["size"][0]*p["size"][1] for k, p in ops if k == "init"]
        assert any(a > b for a, b in zip(sizes, sizes[1:])) and any(a < b for a, b in zip(sizes, sizes[1:]))
        assert len({p["depth"] for k, p in ops if k.startswith("render")}) >= 2

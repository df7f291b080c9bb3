"""CPU tests of the ID-matte boundary (tinsel_hip_render_id_mattes / _device): the declarations and constants in the header, the ctypes
mirror, the kernels in the launch list and in the library under both arithmetic contracts, the refusals that need no GPU, matte and
merge_id_mattes on hand-made lists, the headless options -- and the numpy statement of the rule (tests/id_mattes_reference.py) against code
that is not its own: for random id maps every id's slot weight is, bit for bit, channel x of accumulate_reference.add_passes fed with that
id's indicator, and the total its channel w."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tinsel_amd
from tinsel_amd import abi, headless
from tests.accumulate_reference import add_passes, constructor_offset
from tests.id_mattes_reference import id_mattes, rank

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "tinsel_hip.h")).read()
G = abi.FILTER_GAUSSIAN
FILTERS = {
    "box_1.0": (abi.FILTER_BOX, 1.0, 1.0, constructor_offset(1.0, 1.0)),
    "gauss_0.75": (G, 0.75, 1.0, constructor_offset(0.75, 1.0)),
    "gauss_1.0_loader": (G, 1.0, 1.0, constructor_offset(0.75, 1.0)),        # the loader keeps Filter(gaussian, 0.75, 1.0)'s offset: zero weights
    "gauss_1.5": (G, 1.5, 1.0, constructor_offset(1.5, 1.0)),
    "gauss_2.5": (G, 2.5, 1.0, constructor_offset(2.5, 1.0)),
}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_entries_and_the_constants_are_declared_exported_and_bound():
    L = tinsel_amd.load_library()
    for name, value, mirror in (("TINSEL_ID_MISS", r"\(-1\)", abi.ID_MISS), ("TINSEL_ID_EMPTY", r"\(-2\)", abi.ID_EMPTY), ("TINSEL_ID_MAX_SLOTS", "8", abi.ID_MAX_SLOTS)):
        m = re.search(r"#define %s\s+%s(\s|$)" % (name, value), HEADER)
        assert m, name
        assert mirror == int(value.strip("\\()").replace("\\", ""))
    for name, tail in (("tinsel_hip_render_id_mattes", r"int32_t\* out_ids_host, float\* out_weights_host"),
                       ("tinsel_hip_render_id_mattes_device", r"int32_t\* out_ids_dev, float\* out_weights_dev, void\* stream")):
        assert hasattr(L, name) and name in tinsel_amd.renderer.EXPORTED_SYMBOLS
        assert re.search(r"\bint %s\(tinsel_hip\* r, const tinsel_camera\* camera, const tinsel_options\* options,\s*uint32_t pass_begin, int passes, "
                         r"int slots, %s\);" % (name, tail), HEADER), name
    host, dev = L.tinsel_hip_render_id_mattes.argtypes, L.tinsel_hip_render_id_mattes_device.argtypes
    assert len(host) == 8 and len(dev) == 9 and dev[:8] == host and dev[8] is C.c_void_p
    assert host[3] is C.c_uint32 and host[4] is C.c_int and host[5] is C.c_int and host[0] is host[6] is host[7] is C.c_void_p
    assert callable(tinsel_amd.HipRenderer.id_mattes) and callable(tinsel_amd.matte) and callable(tinsel_amd.merge_id_mattes)
    # the header states the rule, the buffer sizes and where the kernels are timed
    for text in ("total += w", "the FIRST empty slot takes (id, w)", "residual += w", "weight descending, ties by ascending id as int32, empty slots last",
                 "w == +0", "out_ids[slots][H][W]", "out_weights[slots + 2][H][W]", "4 bytes per path slot of a batch", "72 bytes per",
                 "max(1, floor(batch_paths / slots", "have no class there", 'timed under the name "k_features"', "PARTIAL list"):
        assert text in HEADER, text


def test_the_kernels_are_in_the_library_under_both_arithmetic_contracts():
    blob = open(tinsel_amd.renderer.LIB_PATH, "rb").read()
    for ns in (b"_ZN2tn", b"_ZN7tn_fast"):
        assert ns + b"5k_idsILb1EEE" in blob and ns + b"5k_idsILb0EEE" in blob
    # the gather and the ranking: one arithmetic (fp32 adds, one multiply), launched from the exact translation unit
    for kernel in (b"_ZN2tn16k_ids_accumulateE", b"_ZN2tn22k_ids_accumulate_tiledILi3EEE", b"_ZN2tn22k_ids_accumulate_tiledILi4EEE",
                   b"_ZN2tn22k_ids_accumulate_tiledILi0EEE", b"_ZN2tn10k_ids_rankE"):
        assert kernel in blob, kernel
    launch = open(os.path.join(ROOT, "tinsel_amd", "csrc", "tn_launch.h")).read()
    assert re.search(r"X\(PK_IDS_LDS,\s+kBlock, 0, FEATURES,\s*k_ids<true>\)", launch)
    assert re.search(r"X\(PK_IDS,\s+kBlock, 0, FEATURES,\s*k_ids<false>\)", launch)
    kernels = open(os.path.join(ROOT, "tinsel_amd", "csrc", "tn_kernels.h")).read()
    api = open(os.path.join(ROOT, "tinsel_amd", "csrc", "tinsel_hip.hip")).read()
    assert '#include "tn_ids.h"' in kernels and kernels.index('#include "tn_features.h"') < kernels.index('#include "tn_ids.h"')
    assert '#include "tn_host_ids.h"' in api and api.index('#include "tn_host_features.h"') < api.index('#include "tn_host_ids.h"')
    # the name table has not grown: k_ids is timed as k_features, the gather and the ranking have no class
    layout = open(os.path.join(ROOT, "tinsel_amd", "csrc", "tn_host_layout.h")).read()
    names = [s.strip() for s in re.search(r"kKernelNames\[\] = \{([^}]*)\}", layout).group(1).replace('"', "").split(",")]
    assert names[-1] == "k_features" and not any("ids" in n for n in names)
    ids = open(os.path.join(ROOT, "tinsel_amd", "csrc", "tn_ids.h")).read()
    assert "atomic" not in ids.split("#pragma once")[1]


def test_refusals_that_need_no_gpu():
    """(the arguments are judged before the renderer is looked at: a handle that is only non-null will do -- zeroed, it was never init-ed)"""
    L = tinsel_amd.load_library()
    ids, weights = np.full(8*4*4, 5, np.int32), np.full(10*4*4, 5.0, np.float32)
    ip, wp = ids.ctypes.data_as(C.c_void_p), weights.ctypes.data_as(C.c_void_p)
    handle = C.create_string_buffer(1 << 20)
    cam, opt, normals = abi.Camera(), abi.Options(), abi.Options()
    opt.mode, opt.width, opt.height = abi.MODE_PATHTRACE, 4, 4
    normals.mode, normals.width, normals.height = abi.MODE_NORMALS, 4, 4
    cp, opp = C.byref(cam), C.byref(opt)
    host = lambda *a: L.tinsel_hip_render_id_mattes(*a)
    dev = lambda *a: L.tinsel_hip_render_id_mattes_device(*a, None)
    for fn, own in ((host, b"render_id_mattes:"), (dev, b"render_id_mattes_device:")):
        cases = [
            (b"null", (None, cp, opp, 0, 1, 6, ip, wp)),
            (b"null", (handle, None, opp, 0, 1, 6, ip, wp)),
            (b"null", (handle, cp, None, 0, 1, 6, ip, wp)),
            (b"null", (handle, cp, opp, 0, 1, 6, None, wp)),
            (b"null", (handle, cp, opp, 0, 1, 6, ip, None)),
            (b"passes", (handle, cp, opp, 0, 0, 6, ip, wp)),
            (b"passes", (handle, cp, opp, 5, -1, 6, ip, wp)),
            (b"slots", (handle, cp, opp, 0, 1, 0, ip, wp)),
            (b"slots", (handle, cp, opp, 0, 1, 9, ip, wp)),
            (b"slots", (handle, cp, opp, 0, 1, -3, ip, wp)),
            (b"mode", (handle, cp, C.byref(normals), 0, 1, 6, ip, wp)),
            (b"tinsel_hip_init", (handle, cp, opp, 0, 1, 6, ip, wp)),        # no init
        ]
        for cause, case in cases:
            assert L.tinsel_hip_init(None, 0, 0) == -1 and L.tinsel_hip_last_error().startswith(b"init:")      # another entry's text in between
            assert fn(*case) == -1, case
            msg = L.tinsel_hip_last_error()
            assert msg.startswith(own) and cause in msg, msg
            assert (ids == 5).all() and (weights == 5.0).all()


def _result(ids, weights, residual, total):
    return {"ids": np.array(ids, np.int32), "weights": np.array(weights, np.float32), "residual": np.array(residual, np.float32),
            "total": np.array(total, np.float32)}


def test_matte_on_hand_made_lists():
    # one row of four pixels, three slots: [7: 2, 3: 1, miss: 1], [3: 0.5, empty, empty], nothing at all, [miss: 4, 7: 1 + a residual of 3]
    E, M = abi.ID_EMPTY, abi.ID_MISS
    res = _result([[[7, 3, E, M]], [[3, E, E, 7]], [[M, E, E, E]]], [[[2, 0.5, 0, 4]], [[1, 0, 0, 1]], [[1, 0, 0, 0]]], [[0, 0, 0, 3]], [[4, 0.5, 0, 8]])
    m = tinsel_amd.matte(res, 7)
    assert m.dtype == np.float32 and m.shape == (1, 4) and np.array_equal(m, [[0.5, 0, 0, 0.125]])
    assert np.array_equal(tinsel_amd.matte(res, [3]), [[0.25, 1, 0, 0]])
    assert np.array_equal(tinsel_amd.matte(res, (7, 3)), [[0.75, 1, 0, 0.125]])
    assert np.array_equal(tinsel_amd.matte(res, M), [[0.25, 0, 0, 0.5]])
    # an empty slot is no object; an id nobody holds covers nothing; a total of 0 gives 0, not NaN
    assert not tinsel_amd.matte(res, E).any() and not tinsel_amd.matte(res, 99).any()
    assert np.isfinite(tinsel_amd.matte(res, (7, 3, M))).all()
    assert np.array_equal(tinsel_amd.matte(res, (7, 3, M)), [[1, 1, 0, 0.625]])


def test_merge_id_mattes_on_hand_made_lists():
    E, M = abi.ID_EMPTY, abi.ID_MISS
    # two ranks, two slots each, one row of three pixels
    a = _result([[[4, 9, E]], [[2, E, E]]], [[[3, 1, 0]], [[1, 0, 0]]], [[0.5, 0, 0]], [[4.5, 1, 0]])
    b = _result([[[2, 9, M]], [[M, 1, E]]], [[[2.5, 2, 6]], [[2, 2, 0]]], [[0, 0.25, 0]], [[4.5, 4.25, 6]])
    m = tinsel_amd.merge_id_mattes([a, b], 3)
    assert m["ids"].dtype == np.int32 and m["weights"].dtype == np.float32 and m["ids"].shape == m["weights"].shape == (3, 1, 3)
    # pixel 0: 4: 3, 2: 1 + 2.5, miss: 2 -> [2: 3.5, 4: 3, miss: 2]; pixel 1: 9: 1 + 2, 1: 2 -> [9: 3, 1: 2]; pixel 2: [miss: 6]
    assert np.array_equal(m["ids"][:, 0, :], [[2, 9, M], [4, 1, E], [M, E, E]])
    assert np.array_equal(m["weights"][:, 0, :], [[3.5, 3, 6], [3, 2, 0], [2, 0, 0]])
    assert np.array_equal(m["residual"], [[0.5, 0.25, 0]]) and np.array_equal(m["total"], [[9, 5.25, 6]])
    # fewer slots than ids: what does not fit goes to the residual; equal weights rank by ascending id
    m2 = tinsel_amd.merge_id_mattes([a, b], 1)
    assert np.array_equal(m2["ids"], [[[2, 9, M]]]) and np.array_equal(m2["weights"], [[[3.5, 3, 6]]])
    assert np.array_equal(m2["residual"], [[0.5 + 3 + 2, 0.25 + 2, 0]]) and np.array_equal(m2["total"], m["total"])
    tie = tinsel_amd.merge_id_mattes([_result([[[5]], [[E]]], [[[1]], [[0]]], [[0]], [[1]]), _result([[[3]], [[M]]], [[[1]], [[1]]], [[0]], [[2]])], 3)
    assert np.array_equal(tie["ids"][:, 0, 0], [M, 3, 5]) and np.array_equal(tie["weights"][:, 0, 0], [1, 1, 1])
    # more slots than the ranks hold: padded with empty ones; one rank alone is its own list
    wide = tinsel_amd.merge_id_mattes([a], 4)
    assert np.array_equal(wide["ids"][:, 0, :], [[4, 9, E], [2, E, E], [E, E, E], [E, E, E]]) and np.array_equal(wide["residual"], a["residual"])
    # every pixel: slots + residual == total when the inputs were
    for r in (m, m2, wide):
        assert np.array_equal(r["weights"].sum(axis=0) + r["residual"], r["total"])


def test_the_headless_options():
    cfg = headless.parse_args(["headless", "-mattes=m.npz", "-mattes_spp=5", "-mattes_slots=3", "-spp=8", "scene.pack"])
    assert (cfg["mattes"], cfg["mattes_spp"], cfg["mattes_slots"]) == ("m.npz", 5, 3) and cfg["over"] == {"spp": 8}
    cfg = headless.parse_args(["headless", "-mattes=m.npz", "scene.pack"])
    assert cfg["mattes_spp"] is None and cfg["mattes_slots"] is None        # min(spp, 16) passes as -features_spp, 6 slots
    assert headless.parse_args(["headless", "scene.pack"])["mattes"] is None
    for bad in ("-mattes_spp=0", "-mattes_spp=-2", "-mattes_slots=0", "-mattes_slots=9"):
        with pytest.raises(SystemExit):
            headless.parse_args(["headless", "-mattes=m.npz", bad, "scene.pack"])
    # refused where -features is refused, before the scene is opened
    for other in ("-resume=s.npz", "-complexity=rays", "-irradiance=i.npz", "-firsthit=b.npz"):
        with pytest.raises(SystemExit, match="-mattes writes"):
            headless.main(["headless", "-mattes=m.npz", other, "no_such_scene.pack"])
    with pytest.raises(SystemExit, match="-mattes writes"):
        headless.main(["headless", "-mattes=m.npz", "-probes=p.npz", "-probes_at=at.npy", "no_such_scene.pack"])
    with pytest.raises(SystemExit, match="-mattes writes"):
        headless.main(["headless", "-mattes=m.npz", "no_such_%d.pack"])
    for lone in ("-mattes_spp=4", "-mattes_slots=4"):
        with pytest.raises(SystemExit, match="go with -mattes"):
            headless.main(["headless", lone, "no_such_scene.pack"])
    assert "-mattes=FILE.npz" in headless.__doc__ and "-mattes_spp" in headless.__doc__ and "-mattes_slots" in headless.__doc__


# ---------------------------------------------------------------------------
# the numpy statement against AddSample in numpy (code that is not its own)

W, H, PASSES = 23, 17, 3
SEEDS = (0x1234567, 0x89abcdef, 42)


def _random_ids(seed, count):
    """[PASSES, H, W] ids drawn from `count` values, the miss among them, in patches so that neighbours often agree"""
    rng = np.random.default_rng(seed)
    values = np.concatenate([[abi.ID_MISS], rng.choice(200, count - 1, replace=False)]).astype(np.int32)
    coarse = rng.integers(0, count, (PASSES, (H + 2)//3, (W + 2)//3))
    fine = np.repeat(np.repeat(coarse, 3, axis=1), 3, axis=2)[:, :H, :W]
    noise = rng.integers(0, count, (PASSES, H, W))
    return values[np.where(rng.random((PASSES, H, W)) < 0.3, noise, fine)], values


@pytest.mark.parametrize("filt", sorted(FILTERS))
def test_the_statement_is_add_passes_id_by_id(filt):
    path_ids, values = _random_ids(sorted(FILTERS).index(filt), 8)
    got = id_mattes(path_ids, SEEDS, FILTERS[filt], 8)
    assert not got["residual"].any() and (got["ids"] != abi.ID_EMPTY).sum(axis=0).max() >= 3
    total = None
    for v in values:
        radiance = np.zeros((PASSES, H, W, 4), np.float32)
        radiance[..., 0] = path_ids == v
        plane = add_passes(np.zeros((H, W, 4), np.float32), radiance, SEEDS, FILTERS[filt], np.inf)
        held = got["ids"] == v
        assert held.sum(axis=0).max() <= 1
        mine = np.where(held, got["weights"], np.float32(0)).sum(axis=0, dtype=np.float32)
        assert np.array_equal(_bits(mine), _bits(plane[..., 0])), (filt, int(v))
        # a slot is held exactly where the id has weight
        assert np.array_equal(held.any(axis=0), plane[..., 0] > 0)
        total = plane[..., 3]
    assert np.array_equal(_bits(got["total"]), _bits(total)) and total.min() > 0
    # ranked: weights descend, equal weights by ascending id, empty slots last with weight 0
    w, i = got["weights"], got["ids"]
    assert (w[:-1] >= w[1:]).all() and ((w[:-1] > w[1:]) | (i[:-1] < i[1:]) | (i[1:] == abi.ID_EMPTY)).all()
    assert ((i == abi.ID_EMPTY) == (w == 0)).all()
    if filt == "gauss_1.0_loader":
        # candidates of weight +0 exist here and claim nothing (the offset is a narrower filter's)
        assert (FILTERS[filt][3] > constructor_offset(1.0, 1.0))


def test_the_statement_overflows_into_the_residual_in_visiting_order():
    path_ids, values = _random_ids(11, 8)
    full = id_mattes(path_ids, SEEDS, FILTERS["gauss_1.5"], 8, ranked=False)
    for slots in (1, 2, 5):
        cut = id_mattes(path_ids, SEEDS, FILTERS["gauss_1.5"], slots, ranked=False)
        # the first `slots` ids seen keep their slots and their sums; the total does not know about slots
        assert np.array_equal(cut["ids"], full["ids"][:slots]) and np.array_equal(_bits(cut["weights"]), _bits(full["weights"][:slots]))
        assert np.array_equal(_bits(cut["total"]), _bits(full["total"]))
        assert ((cut["residual"] > 0) == (full["ids"][slots:] != abi.ID_EMPTY).any(axis=0)).all() and cut["residual"].any()
    # an ownership mask: the two halves' totals are the whole's where only one half reaches
    left = np.zeros((H, W), bool)
    left[:, :W//2] = True
    a, b = (id_mattes(path_ids, SEEDS, FILTERS["box_1.0"], 8, owned=m) for m in (left, ~left))
    whole = id_mattes(path_ids, SEEDS, FILTERS["box_1.0"], 8)
    assert np.array_equal(a["total"] + b["total"], whole["total"]) and a["total"][:, -1].max() == 0 and b["total"][:, 0].max() == 0
    merged = tinsel_amd.merge_id_mattes([a, b], 8)
    for k in ("ids", "weights", "residual", "total"):           # (box weights are small integers: exact in any order)
        assert np.array_equal(merged[k], whole[k]), k
    ri, rw = rank(full["ids"], full["weights"])
    li, lw = tinsel_amd.rank_id_lists(full["ids"], full["weights"])
    assert np.array_equal(ri, li) and np.array_equal(rw, lw)

"""The traversal-cost map (tinsel_hip_render_cost, kernel k_cost): per pixel and per frame against the C restatement's counters
(PortOracle.render_seeded_counts), pass ranges, shards, no side effects on the renderer, the device's detail counters of every
pipeline against the map, argument checks and the headless -complexity view."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tinsel_amd import abi
from tests import oracle_api as oa

# (mesh:...: generated mesh-heavy scenes, tests/golden/make_mesh_scenes.py -- 12 meshes of 9 ... 5,000 triangles; 80 primitives, 3 of them meshes)
SCENES = ["cornell", "features", "many_spheres", "motionblur", "glass", "ajax_standin_96", "fuzz:03", "fuzz:11", "fuzz:24", "mesh:twelve:1", "mesh:beyond_flat:1"]
KEYS = ("rays", "internal_visits", "tri_tests", "prim_tests")
THREADS = 16


def _pack(name):
    if name.startswith("mesh:"):
        from tests.test_gpu_mesh_scenes import pack_bytes
        return pack_bytes(name)
    if name.startswith("fuzz:"):
        return bytes(np.load(os.path.join(oa.GOLDEN, "fuzz.golden.npz"))["pack_" + name[5:]].tobytes())
    with open(os.path.join(oa.GOLDEN, name + ".pack"), "rb") as fh:
        return fh.read()


@pytest.fixture(scope="module")
def port():
    if not oa.have_port():
        subprocess.run(["make", "-C", os.path.join(oa.ROOT, "oracle"), "port"], check=True)
    return oa.PortOracle()


def _setup(name, W, H):
    import tinsel_amd
    scene = tinsel_amd.Scene(_pack(name))
    cam, opt = abi.Camera.from_buffer_copy(scene.camera), abi.Options.from_buffer_copy(scene.options)
    opt.width, opt.height = W, H
    return scene, cam, opt


def _renderer(scene, opt):
    import tinsel_amd
    r = tinsel_amd.create_gpu_renderer(scene)
    r.init(opt.width, opt.height)
    return r


def _oracle_counts(P, name, cam, opt, pass_begin, passes, window=None):
    h = P.load_pack(_pack(name))
    try:
        _, c, _ = P.render_seeded_counts(h, cam, opt, pass_begin, passes, window=window, threads=1 if window else THREADS)
    finally:
        P.free(h)
    return np.array([c[k] for k in KEYS], np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_per_pixel_equals_the_oracle(port, name):
    scene, cam, opt = _setup(name, 16, 12)
    r = _renderer(scene, opt)
    m = r.render_cost(cam, opt, 0, 2)
    r.close()
    assert m.shape == (12, 16, 4) and m.dtype == np.uint32
    h = port.load_pack(_pack(name))
    bad = []
    try:
        for j in range(12):
            for i in range(16):
                _, c, _ = port.render_seeded_counts(h, cam, opt, 0, 2, window=(i, j, i + 1, j + 1), threads=1)
                want = [c[k] for k in KEYS]
                if list(m[j, i]) != want:
                    bad.append(((i, j), list(m[j, i]), want))
    finally:
        port.free(h)
    assert not bad, "%d pixels differ, first: %s" % (len(bad), bad[:3])


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_frame_totals_equal_the_oracle(port, name):
    scene, cam, opt = _setup(name, 64, 48)
    r = _renderer(scene, opt)
    m = r.render_cost(cam, opt, 0, 4)
    r.close()
    want = _oracle_counts(port, name, cam, opt, 0, 4)
    assert np.array_equal(m.reshape(-1, 4).sum(axis=0, dtype=np.uint64), want)
    assert (m[..., 0] >= 4).all()           # every path traces at least its camera ray


@pytest.mark.gpu
def test_pass_ranges(port):
    name = "features"
    scene, cam, opt = _setup(name, 32, 24)
    r = _renderer(scene, opt)
    a = r.render_cost(cam, opt, 0, 3)
    b = r.render_cost(cam, opt, 3, 2)
    whole = r.render_cost(cam, opt, 0, 5)
    # a request split into several batches (the slot limit) is the same map
    r.set_batch_paths(1024)
    split = r.render_cost(cam, opt, 0, 5)
    r.close()
    assert np.array_equal(b.reshape(-1, 4).sum(axis=0, dtype=np.uint64), _oracle_counts(port, name, cam, opt, 3, 2))
    assert np.array_equal(whole, a + b)
    assert np.array_equal(split, whole)
    assert not np.array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", [abi.PIPELINE_AUTO, abi.PIPELINE_MEGAKERNEL], ids=["auto", "mega"])
def test_no_side_effects(pipeline):
    scene, cam, opt = _setup("cornell", 32, 24)
    r = _renderer(scene, opt)
    r.set_pipeline(pipeline)
    r.set_detail_counters(True)
    r.render(cam, opt, passes=3)
    before = (r.read_accum(), r.get_pass_index(), r.stats())
    m = r.render_cost(cam, opt, 7, 2)
    after = (r.read_accum(), r.get_pass_index(), r.stats())
    assert m.any()
    assert np.array_equal(before[0], after[0]) and before[1:] == after[1:]
    out = r.render(cam, opt, passes=2)
    r.close()

    fresh = _renderer(scene, opt)
    fresh.set_pipeline(pipeline)
    fresh.set_detail_counters(True)
    fresh.render(cam, opt, passes=3)
    ref = fresh.render(cam, opt, passes=2)
    fresh.close()
    assert np.array_equal(out, ref)


@pytest.mark.gpu
def test_pass_begin_means_the_same_wherever_the_generator_stands():
    """render_cost and features of passes 5 and 6 take Random(1) advanced 5 times from the renderer's generator where it has not gone past
    pass 5, else from the seed: every renderer below gives the same bits.  The generator moves only with a render call that the seed table
    does not cover (the first, a rewind in front of the table, 1024 passes on), to that call's first pass: `fresh`, `rendered` and `back`
    leave it at 0, `past` takes it to 9 (the restart from the seed) and `rewound` back to 2 (the advance from a generator that has moved)."""
    scene, cam, opt = _setup("cornell", 50, 37)
    opt.max_depth = 3

    def made(*script):
        r = _renderer(scene, opt)
        for index, passes in script:
            if index is not None:
                r.set_pass_index(index)
            r.render(cam, opt, passes=passes)
        return r

    def side_passes(r):
        return r.render_cost(cam, opt, 5, 2), r.features(cam, opt, 5, 2)

    rendered = made((None, 9))
    renderers = {"fresh": made(), "rendered": rendered, "back": made((None, 9), (2, 1)), "past": made((9, 1)), "rewound": made((9, 1), (2, 1))}
    try:
        got = {k: side_passes(r) for k, r in renderers.items()}
        beauty = rendered.render(cam, opt, passes=2).copy()
        assert rendered.get_pass_index() == 11
    finally:
        for r in renderers.values():
            r.close()
    cost, planes = got["fresh"]
    assert cost.dtype == np.uint32 and cost.any() and all(p.any() for p in planes.values())
    for k, (c, f) in got.items():
        assert np.array_equal(c, cost), k
        assert list(f) == list(planes)
        for n in planes:
            assert np.array_equal(np.ascontiguousarray(f[n]).view(np.uint32), np.ascontiguousarray(planes[n]).view(np.uint32)), (k, n)
    # the calls left the renderer's own passes 9 and 10 what they are without them
    plain = made((None, 9))
    try:
        assert np.array_equal(beauty, plain.render(cam, opt, passes=2))
    finally:
        plain.close()


@pytest.mark.gpu
def test_shards_sum_to_the_unsharded_map():
    scene, cam, opt = _setup("many_spheres", 64, 48)
    r = _renderer(scene, opt)
    whole = r.render_cost(cam, opt, 0, 2)
    r.close()
    world, tile = 3, 16
    tiles_x = (64 + tile - 1)//tile
    jj, ii = np.mgrid[0:48, 0:64]
    owner = ((jj//tile)*tiles_x + ii//tile) % world
    total = np.zeros_like(whole)
    for rank in range(world):
        r = _renderer(scene, opt)
        r.set_shard(rank, world, tile)
        m = r.render_cost(cam, opt, 0, 2)
        r.close()
        assert not m[owner != rank].any(), "rank %d wrote pixels it does not own" % rank
        assert np.array_equal(m[owner == rank], whole[owner == rank])
        total += m
    assert np.array_equal(total, whole)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "features", "ajax_standin_96", "motionblur"])
def test_detail_counters_of_every_pipeline_agree(name):
    scene, cam, opt = _setup(name, 48, 32)
    r = _renderer(scene, opt)
    m = r.render_cost(cam, opt, 0, 3)
    r.close()
    sums = m.reshape(-1, 4).sum(axis=0, dtype=np.uint64)
    for pipeline in (abi.PIPELINE_WAVEFRONT, abi.PIPELINE_WAVEFRONT_SPLIT, abi.PIPELINE_MEGAKERNEL):
        r = _renderer(scene, opt)
        r.set_pipeline(pipeline)
        r.set_detail_counters(True)
        r.render(cam, opt, passes=3)
        st = r.stats()
        r.close()
        got = [st["rays"], st["internal_visits"], st["tri_tests"], st["prim_tests"]]
        assert got == [int(v) for v in sums], "pipeline %d: stats %s, map %s" % (pipeline, got, list(sums))


@pytest.mark.gpu
def test_bad_arguments():
    import ctypes as C
    from tinsel_amd.renderer import TinselHipError, load_library
    scene, cam, opt = _setup("cornell", 16, 12)
    r = _renderer(scene, opt)
    L = load_library()
    out = np.zeros((12, 16, 4), np.uint32)
    ptr = out.ctypes.data_as(C.c_void_p)

    def call(h, o, passes, p):
        rc = L.tinsel_hip_render_cost(h, C.byref(cam), C.byref(o), 0, passes, p)
        return rc, (L.tinsel_hip_last_error() or b"").decode()

    for h, o, passes, p in ((None, opt, 1, ptr), (r._h, opt, 0, ptr), (r._h, opt, -2, ptr), (r._h, opt, 1, None)):
        rc, msg = call(h, o, passes, p)
        assert rc == -1 and msg
    for mode in (abi.MODE_NORMALS, abi.MODE_COMPLEXITY):
        o = abi.Options.from_buffer_copy(opt)
        o.mode = mode
        rc, msg = call(r._h, o, 1, ptr)
        assert rc == -1 and "mode" in msg
    o = abi.Options.from_buffer_copy(opt)
    o.width = 32
    rc, msg = call(r._h, o, 1, ptr)
    assert rc == -1 and "width" in msg
    with pytest.raises(TinselHipError):
        r.render_cost(cam, o, 0, 1)
    # the drop-in's eComplexity stays what it is in the reference: a render that draws nothing
    o = abi.Options.from_buffer_copy(opt)
    o.mode = abi.MODE_COMPLEXITY
    assert not r.render(cam, o, passes=1).any()
    r.close()
    assert not out.any()


@pytest.mark.gpu
def test_headless_complexity_png(tmp_path):
    from tinsel_amd.display import cost_heatmap, png_bytes, quantize_rgb8
    pack = os.path.join(oa.GOLDEN, "cornell.pack")
    png = tmp_path / "nodes.png"
    env = dict(os.environ, PYTHONPATH=oa.ROOT)
    p = subprocess.run([sys.executable, "-m", "tinsel_amd.headless", "-spp=3", "-width=48", "-height=32", "-complexity=nodes",
                        "-out=%s" % png, pack], cwd=oa.ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "mean per sample: rays=" in p.stdout and " nodes=" in p.stdout and " prims=" in p.stdout

    scene, cam, opt = _setup("cornell", 48, 32)
    opt.max_samples = 3
    r = _renderer(scene, opt)
    m = r.render_cost(cam, opt, 0, 3)
    r.close()
    assert png.read_bytes() == png_bytes(quantize_rgb8(cost_heatmap(m, "nodes", samples=3)))
    mean_nodes = m[..., 1].sum(dtype=np.float64)/(48*32*3)
    assert ("nodes=%.4f" % mean_nodes) in p.stdout

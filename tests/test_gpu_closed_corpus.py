"""The closed FIT instance of k_bounce and its baked form (tn_baked.h, tn_host_bake.h) on the closed-set corpus
(tests/golden/closed.golden.npz, tests/golden/make_closed.py): six scenes the plan gives the closed instance, none of them cornell -- light
tables of 2, 4 and 5 lights with different sample counts, sphere lights, no light, no plane table, sixteen table slots, a ninth slot after
the pair block, primitives 62 and 63, random rotations and non-dyadic scales, a 37 x 29 frame.  Per scene the general kernel, the library's
closed instance and the baked instance render the same passes; all three are held to each other, to the reference results the corpus
recorded and, where oracle/_ref is built, to the live reference: per-path radiance and accumulator, bit for bit.  The module's compiles
share one cache directory, so a scene is compiled once."""
import os

import numpy as np
import pytest

import tinsel_amd
from tinsel_amd import abi, create_gpu_renderer
from tinsel_amd import build as hb
from tests import oracle_api as oa

pytestmark = pytest.mark.gpu

F = abi
INSTALLED = (F.BAKE_COMPILED, F.BAKE_FROM_CACHE)
CLOSED = os.path.join(oa.GOLDEN, "closed.golden.npz")
NAMES = [str(n) for n in np.load(CLOSED)["names"]]


@pytest.fixture(scope="module", autouse=True)
def bake_cache(tmp_path_factory):
    was = os.environ.get(hb.BAKE_CACHE_ENV)
    os.environ[hb.BAKE_CACHE_ENV] = str(tmp_path_factory.mktemp("bake_cache"))
    yield os.environ[hb.BAKE_CACHE_ENV]
    if was is None:
        del os.environ[hb.BAKE_CACHE_ENV]
    else:
        os.environ[hb.BAKE_CACHE_ENV] = was


@pytest.fixture(scope="module")
def corpus():
    return np.load(CLOSED)


def _render(r, cam, opt, first, passes):
    r.init(opt.width, opt.height)
    r.set_pass_index(first)
    out = r.render(cam, opt, passes=passes)
    return out, r.batch_radiance(passes, opt.height, opt.width)


def _three(pack, cam, opt, first, passes, tuning):
    """{"general": the general kernel (bounce_fit = 0), "library": the library's closed instance (bounce_bake = 0), "baked": the baked
    instance (bounce_bake = 1)}, each (accumulator, per-path radiance), on renderers of their own under `tuning`"""
    got = {}
    r = create_gpu_renderer(tinsel_amd.Scene(pack), 0, tuning.replace(bounce_fit=0))
    got["general"] = _render(r, cam, opt, first, passes)
    assert r.bounce_plan()[0] == F.BOUNCE_GENERAL
    r.close()

    r = create_gpu_renderer(tinsel_amd.Scene(pack), 0, tuning.replace(bounce_bake=0))
    got["library"] = _render(r, cam, opt, first, passes)
    assert r.bounce_plan()[0] == F.BOUNCE_FIT_CLOSED and r.bake_status()["launches"] == 0
    r.close()

    r = create_gpu_renderer(tinsel_amd.Scene(pack), 0, tuning.replace(bounce_bake=1))
    st = r.bake()
    assert st["state"] in INSTALLED, st
    got["baked"] = _render(r, cam, opt, first, passes)
    after = r.bake_status()
    assert after["state"] in INSTALLED and after["launches"] > st["launches"], (st, after)
    assert r.bounce_plan()[0] == F.BOUNCE_FIT_CLOSED
    r.close()
    return got


def _assert_same(what, a, b):
    """(accumulator, radiance) twice, bit for bit"""
    assert np.array_equal(a[1], b[1]), "%s: %d of %d paths differ" % (what, int((a[1] != b[1]).any(axis=-1).sum()), a[1].size//3)
    assert np.array_equal(a[0], b[0]), "%s: %d pixels of the accumulator differ" % (what, int((a[0] != b[0]).any(axis=-1).sum()))


def _live_reference(pack, cam, opt, first, passes):
    if not oa.have_ref():
        return None
    R = oa.RefOracle()
    h = R.load_pack(pack)
    accum, rad, _ = R.render_seeded(h, cam, opt, first, passes, want_accum=True, want_radiance=True)
    R.free(h)
    return accum, rad


def _hold(name, got, references):
    for kind, pic in got.items():
        assert np.isfinite(pic[0]).all() and np.isfinite(pic[1]).all() and pic[1].any(), "%s, %s" % (name, kind)
    _assert_same("%s: baked against the library's closed instance" % name, got["baked"], got["library"])
    _assert_same("%s: the library's closed instance against the general kernel" % name, got["library"], got["general"])
    _assert_same("%s: baked against the general kernel" % name, got["baked"], got["general"])
    for ref_name, ref in references:
        for kind in ("baked", "library", "general"):
            _assert_same("%s: %s against %s" % (name, kind, ref_name), got[kind], ref)


@pytest.mark.parametrize("name", NAMES)
def test_general_library_and_baked_reproduce_the_reference(corpus, name):
    k = NAMES.index(name)
    pack = corpus["pack_%d" % k].tobytes()
    scene = tinsel_amd.Scene(pack)
    cam, opt = scene.camera, scene.options
    first, passes = int(corpus["first_pass_%d" % k]), int(corpus["passes"])
    got = _three(pack, cam, opt, first, passes, abi.Tuning(bounce_share=0, batch_paths=1 << 22))
    references = [("the corpus's recorded reference", (corpus["accum_%d" % k], corpus["radiance_%d" % k]))]
    live = _live_reference(pack, cam, opt, first, passes)
    if live is not None:
        references.append(("the live reference", live))
    _hold(name, got, references)


# scene: (tuning, passes, held to the live reference too) -- 1024 x 1024 in one batch at the plan's own cut: thousands of regions, several per
# workgroup, the light cursor carried from one to the next.  The default plan shares a workgroup's regions among its waves where a path casts
# three or more shadow rays or the regions are 512 paths or shorter (trace_fused), and shared regions run the general kernel.  two-lights
# casts five shadow rays, and one pass of this frame is cut into regions of 256: its regions are kept apart by the tuning, everything else is
# the default.  sixty-four casts two, and three passes give regions of 768: there the default tuning picks the closed instance by itself, as
# in tests/test_gpu_bake.py::test_cornell_at_the_plans_own_cut (the three kernels against each other only: the reference would take longer
# than everything else in this file).
LARGE = {
    "two-lights": (lambda: abi.Tuning(bounce_share=0), 1, True),
    "sixty-four": (lambda: abi.Tuning(), 3, False),
}


@pytest.mark.parametrize("name", list(LARGE))
def test_a_large_frame_at_the_plans_own_cut(corpus, name):
    tuning, passes, held = LARGE[name]
    k = NAMES.index(name)
    pack = corpus["pack_%d" % k].tobytes()
    scene = tinsel_amd.Scene(pack)
    cam, opt = scene.camera, scene.options.copy()
    opt.width, opt.height = 1024, 1024
    got = _three(pack, cam, opt, 0, passes, tuning())
    live = _live_reference(pack, cam, opt, 0, passes) if held else None
    _hold(name, got, [("the live reference", live)] if live is not None else [])

"""Closed-set corpus (tests/golden/closed.golden.npz, made by the reference from the six scenes of tests/golden/make_closed.py) without a
device: every scene is one the plan gives the closed FIT instance, its generated header states the table shapes the generator worked out
from the scene it wrote, the C restatement reproduces the recorded results bit for bit, and every scene's baked unit cross-compiles for
gfx950 within the closed instance's budget -- a scene whose kernel were refused would leave tests/test_gpu_closed_corpus.py nothing to
compare."""
import json
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import tinsel_amd
from tinsel_amd import abi
from tinsel_amd import build as hb
from tests import oracle_api as oa

CLOSED = os.path.join(oa.GOLDEN, "closed.golden.npz")
NAMES = [str(n) for n in np.load(CLOSED)["names"]]
# the shapes the corpus was asked to have: (plane-table slots, end of the pair blocks, lights, light samples)
SHAPES = {
    "two-lights": (8, 8, 2, 5),
    "four-sphere-lights": (9, 8, 4, 7),
    "five-lights": (8, 8, 5, 8),
    "no-light": (0, 0, 0, 0),
    "sixty-four": (8, 8, 2, 2),
    "thirteen-planes": (16, 8, 2, 3),
}


@pytest.fixture(scope="module")
def corpus():
    return np.load(CLOSED)


def _scene(corpus, name):
    return tinsel_amd.Scene(corpus["pack_%d" % NAMES.index(name)].tobytes())


def test_the_corpus_holds_the_six_shapes(corpus):
    assert sorted(NAMES) == sorted(SHAPES) and [str(f) for f in corpus["fact_names"]] == ["prims", "planes", "pair_end", "lights", "samples"]
    for k, name in enumerate(NAMES):
        assert tuple(int(v) for v in corpus["facts_%d" % k][1:]) == SHAPES[name], name
        opt = _scene(corpus, name).options
        assert (opt.width, opt.height) == (37, 29) and 3 <= opt.max_depth <= 7 and int(corpus["passes"]) == 3
        rad = corpus["radiance_%d" % k]
        assert rad.shape == (3, 29, 37, 3) and np.isfinite(rad).all() and rad.any(axis=-1).mean() >= 0.5, name
    assert int(corpus["facts_%d" % NAMES.index("sixty-four")][0]) == 64 and int(corpus["scan_mask_%d" % NAMES.index("sixty-four")]) >> 62 == 3


@pytest.mark.parametrize("name", NAMES)
def test_every_scene_is_bakeable_and_its_header_states_the_recorded_tables(corpus, name):
    k = NAMES.index(name)
    scene = _scene(corpus, name)
    assert scene.bounce_slim() and scene.bounce_features() == abi.BOUNCE_SPHERE
    text, _, ok, why = scene.bake_source(abi.Tuning(bounce_share=0))
    assert ok, why
    stated = {n: int(v) for n, v in re.findall(r"constexpr int (\w+) = (-?\d+);", text)}
    prims, planes, pair_end, lights, samples = (int(v) for v in corpus["facts_%d" % k])
    want = {"kNumPrims": prims, "kNumPlanes": planes, "kPlanePairEnd": pair_end, "kNumLights": lights, "kTotalLightSamples": samples}
    assert {n: stated[n] for n in want} == want
    mask = re.search(r"constexpr unsigned long long kScanMask = (0x[0-9a-f]{16})ull;", text)
    assert mask and int(mask.group(1), 16) == int(corpus["scan_mask_%d" % k])
    # the light table itself: (primitive, samples) per light, in primitive order
    table = re.search(r"constexpr uint32_t kLights\[\d+\] = \{([^}]*)\}", text).group(1)
    words = [int(w, 16) for w in re.findall(r"0x([0-9a-f]{8})u", table)]
    p = (abi.Primitive*scene.num_primitives).from_address(scene.desc.primitives)
    lit = [(i, p[i].light_samples) for i in range(scene.num_primitives) if p[i].light_samples > 0]
    assert [(words[4*l], words[4*l + 1]) for l in range(lights)] == lit and sum(s for _, s in lit) == samples


@pytest.mark.skipif(not oa.have_port(), reason="oracle/libtinsel_oracle.so not built")
def test_c_restatement_reproduces_the_corpus(corpus):
    P = oa.PortOracle()
    for k, name in enumerate(NAMES):
        h = P.load_pack(corpus["pack_%d" % k].tobytes())
        cam, opt = P.camera_options(h)
        accum, rad, _ = P.render_seeded(h, cam, opt, int(corpus["first_pass_%d" % k]), int(corpus["passes"]), want_accum=True, want_radiance=True, threads=4)
        P.free(h)
        want = corpus["radiance_%d" % k]
        assert np.array_equal(rad, want), "%s: %d paths differ" % (name, int((rad != want).any(axis=-1).sum()))
        assert np.array_equal(accum, corpus["accum_%d" % k]), "%s framebuffer" % name


@pytest.mark.parametrize("name", NAMES)
def test_every_baked_unit_cross_compiles_within_the_closed_instances_budget(corpus, name):
    """build.baked_refusal on the compiler's own report (-Rpass-analysis=kernel-resource-usage): four waves per SIMD, no scratch, VGPRs <= 128
    -- the condition under which a renderer installs the kernel at all."""
    text, _, ok, why = _scene(corpus, name).bake_source(abi.Tuning(bounce_share=0))
    assert ok, why
    with tempfile.TemporaryDirectory(prefix="tinsel_bake_test_") as tmp:
        header = os.path.join(tmp, "scene.h")
        with open(header, "w") as f:
            f.write(text)
        cmd = hb.bake_command(hb.hipcc(), header, "baked.co", extra=["-Rpass-analysis=kernel-resource-usage"])
        p = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-3000:]
        res = hb._parse_resources(p.stderr).get(hb.BAKED_KERNEL)
        if res:
            res["code_bytes"] = hb._code_bytes(os.path.join(tmp, "baked.co")).get(hb.BAKED_KERNEL)
    print("baked %s of %s:" % (hb.BAKED_KERNEL, name), json.dumps(res, sort_keys=True))
    assert hb.baked_refusal(res) is None, hb.baked_refusal(res)

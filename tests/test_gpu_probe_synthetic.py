"""The two probe samplers on probes the tests build themselves (tests/probe_host.py): nothing under tests/golden/large/ and no oracle/_ref
is needed, so nothing here skips.  Scene geometry is features_probe.pack throughout, its probe replaced by a catalogue probe
(ph.with_probe); frames are 48 x 32, 4 passes unless a test says otherwise.

The yardsticks are not under test: tests/test_probe_host.py holds the model of ProbeSample's choice and the C restatement (port_leaf_probe,
port_render_seeded) to each other and, where oracle/_ref is built, to the reference's own code on these very packs, and checks the
statistical margins used below on a model of the alias sampler with the same seeds.

(a) CDF arm, leaf   (b) alias arm, leaf   (c) CDF arm, renders   (d) alias arm, renders   (e) the alias arm is the same estimator
(f) what is built on a render stays built on it in alias mode."""
import functools

import numpy as np
import pytest

import tinsel_amd
from tinsel_amd import abi
from tests import light_groups_reference as lg
from tests import oracle_api as oa
from tests import probe_host as ph

pytestmark = pytest.mark.gpu

W, H, PASSES = ph.W, ph.H, ph.PASSES
N_LEAF = ph.LEAF_ROWS
# the CDF run an alias row's texel is looked up in has the alias run's seeds -- but on big, where 200,000 draws reach 93.6 % of the mass of
# its 80,000 texels: sum_i p_i*exp(-D*p_i) is 0.065 at D = 200,000, 0.0076 at 1,000,000 and 0.0029 at 2,000,000 (the condition: 0.01)
N_CDF_LOOKUP = {"big": 2_000_000}
PIPELINES = {"auto": abi.PIPELINE_AUTO, "wavefront": abi.PIPELINE_WAVEFRONT, "mega": abi.PIPELINE_MEGAKERNEL, "split": abi.PIPELINE_WAVEFRONT_SPLIT}


def _renderer(name, mode=abi.PROBE_CDF, pipeline=None, width=0, height=0, masked=False):
    b = ph.blob(name)
    scene = tinsel_amd.Scene(lg.masked_pack(b, (), True) if masked else b)
    assert scene.desc.probe_valid and (scene.desc.probe_width, scene.desc.probe_height) == ph.SIZES[name]
    r = tinsel_amd.create_gpu_renderer(scene)
    if pipeline is not None:
        r.set_pipeline(pipeline)
    r.set_probe_sampling(mode)
    if width:
        r.init(width, height)
    return r


@functools.lru_cache(maxsize=None)
def gpu_leaf(name, mode, n):
    """tinsel_hip_leaf's ProbeSample / ProbePdf / Sky::Eval rows of probe `name` on ph.seeds(n), in the given sampling mode"""
    r = _renderer(name, mode)
    try:
        out = r.leaf(6, 0, n, 11, seeds=ph.seeds(n))
    finally:
        r.close()
    out.setflags(write=False)
    return out


def _same(got, want, what):
    a, b = ph.bits(got), ph.bits(want)
    assert a.shape == b.shape, what
    bad = a != b
    assert not bad.any(), "%s: %d of %d words differ (first at %s: %s against %s)" % (
        what, int(bad.sum()), bad.size, np.unravel_index(np.argmax(bad), bad.shape), got[np.unravel_index(np.argmax(bad), bad.shape)],
        want[np.unravel_index(np.argmax(bad), bad.shape)])


# ---------------------------------------------------------------------------
# (a) the CDF arm, leaf

@pytest.mark.parametrize("name", ph.LEAF_PROBES)
def test_cdf_leaf_is_the_model_and_the_restatement(name):
    p = ph.probe(name)
    u1, r1, u2, r2 = ph.draws(ph.seeds(N_LEAF))
    want = ph.cdf_pick(p, r1, r2)
    assert (want < p.n).all()                            # (no seed sends the column search one past its row)
    out = gpu_leaf(name, abi.PROBE_CDF, N_LEAF)
    d, c, pdf, pdf2, ev = ph.port_leaf(name, N_LEAF)
    assert np.array_equal(p.texel_of(out[:, 3:6]), want), "the colour is that of the model's texel on every row"
    _same(out[:, 0:3], d, name + " ProbeSample dir")
    _same(out[:, 3:6], c, name + " ProbeSample colour")
    _same(out[:, 6], pdf, name + " ProbeSample pdf")
    # ProbePdf / Sky::Eval of a texel's CORNER: a 1-ulp uv lands on the neighbouring texel (tests/test_gpu_leaf.py)
    same_pdf = (ph.bits(out[:, 7]) == ph.bits(pdf2)) | (np.isnan(out[:, 7]) & np.isnan(pdf2))          # (0*NaN beside a black row)
    same_ev = (ph.bits(out[:, 8:11]) == ph.bits(ev)).all(axis=1)
    print("%s: ProbePdf(dir) identical on %.5f, Sky::Eval(dir) on %.5f of the rows" % (name, same_pdf.mean(), same_ev.mean()))
    assert same_pdf.mean() >= 0.9999 and same_ev.mean() >= 0.9999
    if len(p.black_rows):
        assert not np.isin(p.texel_of(out[:, 3:6])//p.W, p.black_rows).any()
    if name == "thin_9x1":
        assert (out[:, 6] == 0).all()


# ---------------------------------------------------------------------------
# (b) the alias arm, leaf

@pytest.mark.parametrize("name", ph.LEAF_PROBES)
def test_alias_leaf_draws_the_probes_distribution(name):
    """Measured on an MI355X (the model's figures, on the same seeds, are in tests/test_probe_host.py):

        probe       total bracket width (cap 0.01)    worst texel of the frequency check (of 6 standard deviations)
        flat        0.00448                           3.44
        one         0.00000                           0.00
        thin_7x3    0.00037                           2.90
        thin_1x9    0.00015                           1.54
        thin_9x1    0.00019                           1.28
        blackrows   0.00022                           2.58
        odd         0.00486                           3.41
        big         0.95248  (cap 1.48987)            3.55

    The cap is ph.alias_width_cap: 1 % of the mass, but on big what 200,000 rows over 80,000 bins allow (1.48987), see there.  On big
    the CDF run that an alias row's texel is looked up in has 2,000,000 seeds, see N_CDF_LOOKUP."""
    p = ph.probe(name)
    n = ph.alias_rows(name)
    n_cdf = N_CDF_LOOKUP.get(name, n)
    if n_cdf != N_LEAF:                                  # (test (a) holds the model to the kernel on N_LEAF seeds; this is the model alone)
        u1, r1, u2, r2 = ph.draws(ph.seeds(n_cdf))
        assert (ph.cdf_pick(p, r1, r2) < p.n).all()      # (no seed sends the column search one past its row)
    cdf = gpu_leaf(name, abi.PROBE_CDF, n_cdf)
    out = gpu_leaf(name, abi.PROBE_ALIAS, n)
    t_cdf, t = p.texel_of(cdf[:, 3:6]), p.texel_of(out[:, 3:6])
    # a texel with p_i == 0 (a black row's among them) is never returned: every colour names a positive-probability texel
    assert (t >= 0).all() and (t_cdf >= 0).all() and (p.p[t] > 0).all()
    if len(p.black_rows):
        assert not np.isin(t//p.W, p.black_rows).any()
    # every row is, bit for bit, what the CDF arm returns for the texel the colour names
    first = np.full(p.n, -1, np.int64)
    first[t_cdf[::-1]] = np.arange(n_cdf - 1, -1, -1)
    covered = first[t] >= 0
    print("%s: %.5f of the alias rows name a texel the CDF run drew" % (name, covered.mean()))
    # (all of them where the CDF run expects every texel it can draw 50 times or more: flat, one, the thin ones, blackrows)
    assert covered.mean() >= 0.99 and (covered.all() or n_cdf*p.p[p.p > 0].min() < 50)
    _same(out[covered, 0:7], cdf[first[t[covered]], 0:7], name + " alias rows against the CDF arm's rows of the same texel")
    # the structure of an alias sampler, and the probabilities it implies
    u1, r1, u2, r2 = ph.draws(ph.seeds(n))
    lower, upper, width = ph.alias_structure(u1, r2, t, p.n)
    inside = ph.in_brackets(p.p, lower, upper)
    print("%s: total bracket width %.5f of the mass (cap %.5f)" % (name, width, ph.alias_width_cap(name)))
    assert inside.all(), "%d texels' probabilities lie outside their brackets (first: %d)" % (int((~inside).sum()), int(np.argmin(inside)))
    assert width <= ph.alias_width_cap(name)
    assert ph.frequencies_ok(p.p, t, name)


def test_alias_mode_builds_on_black_rows_and_refuses_a_black_probe():
    r = _renderer("blackrows", abi.PROBE_ALIAS)          # (before the builder's fix: "the probe has no energy")
    r.close()
    black = np.zeros((3, 5, 4), np.float32)
    black[..., 3] = 1.0
    scene = tinsel_amd.Scene(ph.with_probe(lg.pack_bytes("features_probe"), black))
    r = tinsel_amd.create_gpu_renderer(scene)
    try:
        with pytest.raises(Exception, match="the probe has no energy"):
            r.set_probe_sampling(abi.PROBE_ALIAS)
    finally:
        r.close()


# ---------------------------------------------------------------------------
# (c) the CDF arm, renders

@pytest.mark.parametrize("pipeline", sorted(PIPELINES))
@pytest.mark.parametrize("name", ph.RENDER_PROBES)
def test_cdf_render_is_the_restatements_bit_for_bit(name, pipeline):
    acc, rad = ph.port_render(name, radiance=True)
    cam, opt = lg.frame(ph.blob(name), W, H)
    r = _renderer(name, abi.PROBE_CDF, PIPELINES[pipeline], W, H)
    try:
        out = r.render(cam, opt, passes=PASSES)
        got = r.batch_radiance(PASSES, H, W)
    finally:
        r.close()
    _same(got, rad, "%s %s per-path radiance" % (name, pipeline))
    _same(out, acc, "%s %s accumulator" % (name, pipeline))


# ---------------------------------------------------------------------------
# (d) the alias arm, renders

@pytest.mark.parametrize("name", ph.ALIAS_RENDER_PROBES)
def test_alias_render_is_one_image_on_every_pipeline_and_cdf_comes_back(name):
    acc, _ = ph.port_render(name)
    cam, opt = lg.frame(ph.blob(name), W, H)
    images = {}
    for pipeline, value in PIPELINES.items():
        r = _renderer(name, abi.PROBE_ALIAS, value, W, H)
        try:
            images[pipeline] = r.render(cam, opt, passes=PASSES)
            r.set_probe_sampling(abi.PROBE_CDF)
            r.init(W, H)
            r.set_pass_index(0)
            back = r.render(cam, opt, passes=PASSES)
        finally:
            r.close()
        _same(back, acc, "%s %s: the CDF accumulator after set_probe_sampling(PROBE_CDF)" % (name, pipeline))
    for pipeline in PIPELINES:
        assert np.isfinite(images[pipeline]).all()
        _same(images[pipeline], images["auto"], "%s: alias accumulator, %s against auto" % (name, pipeline))
    assert np.array_equal(images["auto"][..., 3], acc[..., 3]) and not np.array_equal(images["auto"][..., :3], acc[..., :3])


# ---------------------------------------------------------------------------
# (e) the alias arm is the same estimator

@pytest.mark.parametrize("name", ["odd", "big"])
def test_alias_render_estimates_what_the_cdf_render_estimates(name):
    """64 x 48, 64 passes.  The yardstick is the existing test's (tests/test_gpu_probe.py): the per-pixel L2 between two CDF renders on
    other passes, and its margin of 1.5.  Measured on an MI355X:

        probe   L2 alias vs CDF   L2 of two CDF renders   ratio (cap 1.5)   mean difference, standard errors (cap 6)
        odd     3.0135e-01        3.7723e-01              0.799             1.06    (the two CDF renders: 1.95)
        big     6.4754e-02        1.2564e-01              0.515             0.36    (the two CDF renders: 1.69)

    The C restatement's two CDF renders alone give the same 1.95 and 1.69 (tests/test_probe_host.py)."""
    w, h, passes = 64, 48, 64
    cam, opt = lg.frame(ph.blob(name), w, h)
    img = {}
    for key, mode, begin in (("cdf", abi.PROBE_CDF, 0), ("alias", abi.PROBE_ALIAS, 0), ("cdf2", abi.PROBE_CDF, 5000)):
        r = _renderer(name, mode, None, w, h)
        try:
            r.set_pass_index(begin)
            img[key] = r.render(cam, opt, passes=passes)
        finally:
            r.close()
        assert np.isfinite(img[key]).all()
    l2, noise = oa.image_l2(img["alias"], img["cdf"]), oa.image_l2(img["cdf"], img["cdf2"])
    z, z_noise = ph.mean_difference_z(img["alias"], img["cdf"]), ph.mean_difference_z(img["cdf"], img["cdf2"])
    print("%s 64x48 @ 64: alias vs cdf L2 %.4e, two cdf renders %.4e (ratio %.3f); mean difference %.2f standard errors (two cdf renders: %.2f)"
          % (name, l2, noise, l2/noise, z, z_noise))
    assert not np.array_equal(img["alias"], img["cdf"])
    assert l2 <= 1.5*noise
    assert z <= 6.0


# ---------------------------------------------------------------------------
# (f) what is built on a render stays built on it in alias mode

def _camera_starts(r, cam, width, height, passes):
    """the records of the frame's own camera paths in slot order (pass, row, column), as tests/test_gpu_radiance_query.py states them, from
    this file's own means: the generator in numpy (tinsel_amd.rng_state) and the device's GenerateRay leaf (bit-identical to the
    reference's, tests/test_gpu_leaf.py)"""
    O = oa.PortOracle()
    jj, ii = np.mgrid[0:height, 0:width]
    i, j = ii.ravel().astype(np.uint32), jj.ravel().astype(np.uint32)
    out = []
    for s in range(passes):
        seed = i + j*np.uint32(width) + np.uint32(O.pass_seed(s))
        x, y, t = ((tinsel_amd.rng_state(seed, k)[0].astype(np.float32)*np.float32(1.0/4294967296.0)) for k in (1, 2, 3))
        raster = np.stack([x + i.astype(np.float32), y + j.astype(np.float32)], axis=1).astype(np.float32)
        od = r.leaf(1, 0, len(raster), 6, rows=raster, camera=cam, width=width, height=height)
        a, b = np.float32(cam.shutter_start), np.float32(cam.shutter_end)
        st = np.zeros(len(raster), abi.PATH_START_DTYPE)
        st["ox"], st["oy"], st["oz"], st["dx"], st["dy"], st["dz"] = (od[:, q] for q in range(6))
        st["time"] = a + (b - a)*t
        st["rng1"], st["rng2"] = tinsel_amd.rng_state(seed, 3)
        out.append(st)
    return np.concatenate(out)


def test_everything_built_on_a_render_follows_the_alias_mode():
    """These identities are pinned in CDF mode by the features' own tests; a shading kernel that ignores the alias table fails here."""
    name, passes = "odd", 2
    cam, opt = lg.frame(ph.blob(name), W, H)
    cdf, _ = ph.port_render(name, passes=passes)
    r = _renderer(name, abi.PROBE_ALIAS, None, W, H)
    try:
        beauty = r.render(cam, opt, passes=passes)
        rad = r.batch_radiance(passes, H, W)
        assert np.isfinite(beauty).all() and not np.array_equal(beauty, cdf)
        got = r.radiance(_camera_starts(r, cam, W, H, passes), opt.max_depth)
        _same(got[:, :3], rad.reshape(-1, 3), "radiance() of the render's own camera paths")
        _same(r.views([cam], opt, 0, passes)[0], beauty, "plane 0 of views with one camera")
        _same(r.sample_map(cam, opt, np.full((H, W), passes, np.uint16), 0), beauty, "a uniform sample map")
        _same(r.depth_planes(cam, opt, 0, passes, depths=[1, opt.max_depth])[-1], beauty, "the deepest depth plane")
        emitters = lg.emitters(ph.blob(name))
        table = np.full(lg.header(ph.blob(name)).num_primitives, -1, np.int32)
        table[emitters] = np.arange(len(emitters))
        planes = r.light_groups(cam, opt, 0, passes, table, len(emitters))
    finally:
        r.close()
    m = _renderer(name, abi.PROBE_ALIAS, None, W, H, masked=True)
    try:
        env = m.render(cam, opt, passes=passes)
    finally:
        m.close()
    assert env[..., :3].any()
    _same(planes[len(emitters)], env, "the environment plane against the alias render of the scene with all emission masked")

"""The host side of the synthetic-probe tests: probes the tests build themselves, the byte edit that gives a committed pack another probe,
and plain statements of what the two probe samplers must do.  No GPU, nothing read from the reference tree, nothing written to disk.

build_cdf       Probe::BuildCDF (probe.h:31-79) in float32 numpy, held bit for bit to the tables of the committed packs
                (tests/test_probe_host.py); an all-black row gets pdfX = 0*inf = NaN and pdfY = 0, as the reference's does.
with_probe      a pack with its five probe sections (the last five of a pack) replaced and the header's offsets, probe size and
                total_bytes rewritten.
catalogue       the probes, each a function of a fixed seed.  Texel colours are distinct among positive-probability texels (asserted),
                so the colour a sampler returns names its texel.
draws           the two draws ProbeSample takes from Random(seed), vectorised; held to port_leaf_random by the host test.
cdf_pick        which texel ProbeSample's two binary searches pick (np.searchsorted, side="left", on the float32 tables).
vose / alias_pick
                a float64 alias table of the tests' own and its selection, the model the statistical margins are checked on.
alias_structure the exact, non-statistical check of an alias sampler's outputs (see its docstring); alias_width_bound: what its width
                may be at a given number of rows.
blob, port_render, port_leaf, model_rows, frequencies_ok, mean_difference_z
                what the host test and the GPU test share: features_probe.pack with a catalogue probe, the C restatement's render and
                leaf rows of it (computed once, read-only), the model's rows, and the two statistics both files assert."""
import ctypes as C
import functools
import os

import numpy as np

from tinsel_amd import abi
from tests import light_groups_reference as lg
from tests import oracle_api as oa


# ---------------------------------------------------------------------------
# BuildCDF

def luminance(texels):
    """Luminance(Color) (maths.h): (r*0.3f + g*0.6f) + b*0.1f in float32"""
    t = np.asarray(texels, np.float32)
    return (t[..., 0]*np.float32(0.3) + t[..., 1]*np.float32(0.6)) + t[..., 2]*np.float32(0.1)


def build_cdf(texels):
    """texels [H, W, 4] float32 -> (pdf_x [H, W], cdf_x [H, W], pdf_y [H], cdf_y [H]), float32, sums in row order, one reciprocal per row"""
    w = luminance(texels)
    assert w.dtype == np.float32 and w.ndim == 2
    cdf_x = np.add.accumulate(w, axis=1, dtype=np.float32)                  # (accumulate is sequential: no pairwise sums)
    total_x = cdf_x[:, -1].copy()
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.float32(1.0)/total_x
        pdf_x = w*inv[:, None]
        cdf_x = cdf_x*inv[:, None]
        cdf_y = np.add.accumulate(total_x, dtype=np.float32)
        total_y = cdf_y[-1]
        pdf_y = total_x/total_y
        cdf_y = cdf_y/total_y
    return pdf_x, cdf_x, pdf_y, cdf_y


# ---------------------------------------------------------------------------
# packs

HEADER_BYTES = C.sizeof(abi.PackHeader)


def header(blob):
    return abi.PackHeader.from_buffer_copy(bytes(blob[:HEADER_BYTES]))


def _align16(n):
    return (n + 15) & ~15


def probe_sections(blob):
    """(texels [H, W, 4], pdf_x, cdf_x, pdf_y, cdf_y) of a pack that has a probe, as copies"""
    h = header(blob)
    W, H = h.probe_width, h.probe_height
    assert h.off_probe_data and W > 0 and H > 0

    def at(off, count):
        return np.frombuffer(blob, np.float32, count, off).copy()
    return (at(h.off_probe_data, W*H*4).reshape(H, W, 4), at(h.off_probe_pdf_x, W*H).reshape(H, W), at(h.off_probe_cdf_x, W*H).reshape(H, W),
            at(h.off_probe_pdf_y, H), at(h.off_probe_cdf_y, H))


def with_probe(blob, texels):
    """The pack with this probe: everything before the probe's texels stays, the five sections follow 16-byte aligned in the writer's
    order (texels, pdf_x, cdf_x, pdf_y, cdf_y), and the total is rounded up to 16."""
    texels = np.ascontiguousarray(texels, np.float32)
    H, W = texels.shape[:2]
    assert texels.shape == (H, W, 4)
    h = header(blob)
    offs = [h.off_probe_data, h.off_probe_pdf_x, h.off_probe_cdf_x, h.off_probe_pdf_y, h.off_probe_cdf_y]
    assert h.off_probe_data and offs == sorted(offs) and h.off_probe_data > max(h.off_primitives, h.off_bvh_nodes), "the probe sections are the last five"
    out = bytearray(blob[:h.off_probe_data])
    new = []
    for section in (texels,) + build_cdf(texels):
        out.extend(bytes(_align16(len(out)) - len(out)))
        new.append(len(out))
        out.extend(np.ascontiguousarray(section, np.float32).tobytes())
    out.extend(bytes(_align16(len(out)) - len(out)))
    h.off_probe_data, h.off_probe_pdf_x, h.off_probe_cdf_x, h.off_probe_pdf_y, h.off_probe_cdf_y = new
    h.probe_width, h.probe_height, h.total_bytes = W, H, len(out)
    out[:HEADER_BYTES] = bytes(h)
    return bytes(out)


# ---------------------------------------------------------------------------
# the catalogue

_KEY = np.dtype([("r", "<u4"), ("g", "<u4"), ("b", "<u4")])


def _keys(rgb):
    return np.ascontiguousarray(rgb, np.float32).reshape(-1, 3).view(np.uint32).view(_KEY).reshape(-1)


class Probe:
    """A probe and what follows from its texels alone.  p [H*W] float64: the selection probability pdfY*pdfX of every texel, normalised,
    0 on a row with pdfY == 0 (an all-black row's pdfX is NaN)."""

    def __init__(self, name, texels):
        self.name = name
        self.texels = np.ascontiguousarray(texels, np.float32)
        self.texels.setflags(write=False)
        self.H, self.W = self.texels.shape[:2]
        self.n = self.W*self.H
        self.pdf_x, self.cdf_x, self.pdf_y, self.cdf_y = build_cdf(self.texels)
        with np.errstate(invalid="ignore"):
            p = np.where(self.pdf_y[:, None] == 0, 0.0, self.pdf_y.astype(np.float64)[:, None]*self.pdf_x.astype(np.float64)).reshape(-1)
        assert np.isfinite(p).all() and p.sum() > 0
        self.p = p/p.sum()
        self.black_rows = np.flatnonzero(self.pdf_y == 0)
        # a returned colour names its texel: distinct among the texels that can be returned
        live = np.flatnonzero(self.p > 0)
        keys = _keys(self.texels[..., :3])[live]
        order = np.argsort(keys)
        self._keys, self._texel = keys[order], live[order]
        assert len(np.unique(self._keys)) == len(live), "%s: two positive-probability texels share a colour" % name

    def texel_of(self, rgb):
        """the flat index row*W + col of the positive-probability texel of this colour, -1 where there is none"""
        k = _keys(rgb)
        at = np.minimum(np.searchsorted(self._keys, k), len(self._keys) - 1)
        return np.where(self._keys[at] == k, self._texel[at], -1)


def _rgba(rgb):
    return np.concatenate([rgb, np.ones(rgb.shape[:2] + (1,), rgb.dtype)], axis=-1).astype(np.float32)


def _odd(rng):
    """50 x 25: random**8 * 4, one texel at 3000 per channel (about 84 % of the energy), column 25 black"""
    t = (rng.random((25, 50, 3))**8*4.0).astype(np.float32)
    t[:, 25] = 0.0
    t[9, 31] = 3000.0
    return t


def _flat(rng):
    """48 x 24: values in [0.5, 1.5]: no texel dominates, and nearly every bin of an alias table splits its draws between two texels"""
    return (0.5 + rng.random((24, 48, 3))).astype(np.float32)


def _big(rng):
    """400 x 200: random**8 * 4 with a bright blob; 80,000 texels, no power of two, searches 8 (rows) and 9 (columns) steps deep"""
    t = rng.random((200, 400, 3))**8*4.0
    jj, ii = np.mgrid[0:200, 0:400]
    t += (60.0*np.exp(-(((ii - 131.0)/9.0)**2 + ((jj - 57.0)/6.0)**2)))[..., None]*(0.5 + rng.random((200, 400, 3)))
    return t.astype(np.float32)


def _blackrows(rng):
    """12 x 6: rows 0, 3 and 5 black (BuildCDF leaves pdfX = NaN and pdfY = 0 there)"""
    t = (0.25 + rng.random((6, 12, 3))).astype(np.float32)
    t[[0, 3, 5]] = 0.0
    return t


# name: (seed, maker); sizes are width x height
_MAKERS = {
    "odd": (101, _odd),
    "flat": (102, _flat),
    "one": (103, lambda rng: (0.5 + rng.random((1, 1, 3))).astype(np.float32)),
    "thin_7x3": (104, lambda rng: (rng.random((3, 7, 3))*2.0).astype(np.float32)),
    "thin_1x9": (105, lambda rng: (rng.random((9, 1, 3))*2.0).astype(np.float32)),
    "thin_9x1": (106, lambda rng: (rng.random((1, 9, 3))*2.0).astype(np.float32)),       # its only row has sinTheta == 0: every pdf is 0
    "big": (107, _big),
    "blackrows": (108, _blackrows),
}
LEAF_PROBES = tuple(_MAKERS)
RENDER_PROBES = ("odd", "flat", "one", "thin_7x3", "big")          # blackrows is never rendered: the reference's own render of it is NaN
ALIAS_RENDER_PROBES = ("odd", "flat", "big")
SIZES = {"odd": (50, 25), "flat": (48, 24), "one": (1, 1), "thin_7x3": (7, 3), "thin_1x9": (1, 9), "thin_9x1": (9, 1), "big": (400, 200),
         "blackrows": (12, 6)}


@functools.lru_cache(maxsize=None)
def probe(name):
    seed, make = _MAKERS[name]
    p = Probe(name, _rgba(make(np.random.default_rng(seed))))
    assert (p.W, p.H) == SIZES[name]
    return p


# ---------------------------------------------------------------------------
# the generator's two draws and the reference sampler's choice

_M32 = np.uint64(0xFFFFFFFF)


def _rotl(x, k):
    return ((x << np.uint64(k)) | (x >> np.uint64(32 - k))) & _M32


def draws(seeds):
    """Random(seed) (maths.h:1036-1091), vectorised: (u1, r1, u2, r2) -- the integer outputs of the first two Rand() calls and the two
    Randf(0, 1) values ProbeSample makes of them, float32."""
    s1 = (np.asarray(seeds).astype(np.uint64) + np.uint64(315645664)) & _M32
    s2 = s1 ^ np.uint64(0x13AB45FE)
    out = []
    for _ in range(2):
        s1 = ((s2 ^ _rotl(s1, 5)) ^ (s1*s2)) & _M32
        s2 = s1 ^ _rotl(s2, 12)
        u = s1.astype(np.uint32)
        t = u.astype(np.float32)*np.float32(1.0/4294967296.0)                       # Randf(): value*(1.0f/float(0xffffffff))
        out += [u, (np.float32(1.0) - t)*np.float32(0.0) + t*np.float32(1.0)]       # Randf(0, 1)
    return tuple(out)


def seeds(n):
    """the leaf tests' seeds: n distinct, fixed"""
    return ((np.arange(1, n + 1, dtype=np.uint64)*np.uint64(2654435761)) % np.uint64(2**32)).astype(np.uint32)


def cdf_pick(p, r1, r2):
    """ProbeSample's texel (probe.h:205-236): LowerBound on cdfY with r1, then on the row's cdfX with r2 -> flat index row*W + col.
    (col == W, one past the row, is what LowerBound returns for an r2 above the row's last cdf value; the flat index says so.)"""
    row = np.searchsorted(p.cdf_y, r1, side="left")
    assert (row < p.H).all()
    col = np.zeros(len(row), np.int64)
    for j in np.unique(row):
        m = row == j
        col[m] = np.searchsorted(p.cdf_x[j], r2[m], side="left")
    return row*p.W + col


# ---------------------------------------------------------------------------
# an alias table of the tests' own

def vose(p):
    """Vose's alias method in float64 over probabilities p (sum 1) -> (keep [n] float32, alias [n] int64): bin k keeps texel k where
    r2 < keep[k] and hands the draw to alias[k] otherwise.  Queues, not stacks: the order is this file's own."""
    n = len(p)
    scaled = np.asarray(p, np.float64)*n
    keep = np.full(n, 2.0, np.float32)              # r2 <= 1 < 2: always keep
    alias = np.arange(n, dtype=np.int64)
    small = [k for k in range(n) if scaled[k] < 1.0]
    large = [k for k in range(n) if scaled[k] >= 1.0]
    scaled = scaled.tolist()
    si = li = 0
    while si < len(small) and li < len(large):
        s, l = small[si], large[li]
        si += 1
        keep[s], alias[s] = scaled[s], l
        scaled[l] = (scaled[l] + scaled[s]) - 1.0
        if scaled[l] < 1.0:
            li += 1
            small.append(l)
    return keep, alias


def alias_pick(keep, alias, u1, r2):
    """the selection of tn_probe.h: bin k from the first draw's 32 integer bits, texel k where r2 < keep[k], else alias[k]"""
    n = len(keep)
    k = ((u1.astype(np.uint64)*np.uint64(n)) >> np.uint64(32)).astype(np.int64)
    return np.where(r2 < keep[k], k, alias[k])


def table_probabilities(keep, alias):
    """the selection probability of every texel that a table realises (float64; r2 taken as uniform on [0, 1))"""
    n = len(keep)
    q = np.minimum(keep.astype(np.float64), 1.0)
    out = q/n
    np.add.at(out, alias, (1.0 - q)/n)
    return out


class AliasStructureError(AssertionError):
    pass


def alias_structure(u1, r2, texel_out, n):
    """What the outputs of an alias sampler over n bins must look like, whatever its table holds -- exact, not statistical.

    Rows are grouped by the bin k = (u1*n) >> 32.  Inside one bin (AliasStructureError otherwise)
      - every row that did not return texel k returns one and the same other texel a_k;
      - the largest r2 among the rows that kept k is below the smallest r2 among the rows that went to a_k.
    So the bin's keep-threshold lies in (lo_k, hi_k], lo_k the former (0 where no row kept) and hi_k the latter (1 where no row went).
    A bin holds 1/n of the draws (to 2^-32*n), so texel i is selected with a probability in [lower_i, upper_i]:
        lower_i = lo_i/n + sum over the bins k with a_k = i of (1 - hi_k)/n
        upper_i = hi_i/n + sum over the bins k with a_k = i of (1 - lo_k)/n + U
    U the mass (1 - lo_k)/n of the bins whose alias was never seen, which may belong to any texel.

    Returns (lower, upper, width): width = sum_i (upper_i - lower_i - U) + U, the probability mass the rows leave undecided, every
    bin's undecided interval (hi_k - lo_k)/n counted twice: once for texel k and once for the texel it may be handed to.

    in_brackets() is the comparison of a probability vector with (lower, upper) and states its slack."""
    u1, r2, texel_out = np.asarray(u1), np.asarray(r2, np.float64), np.asarray(texel_out, np.int64)
    k = ((u1.astype(np.uint64)*np.uint64(n)) >> np.uint64(32)).astype(np.int64)
    kept = texel_out == k
    lo = np.zeros(n)
    hi = np.ones(n)
    np.maximum.at(lo, k[kept], r2[kept])
    np.minimum.at(hi, k[~kept], r2[~kept])
    a_min = np.full(n, np.iinfo(np.int64).max)
    a_max = np.full(n, -1)
    np.minimum.at(a_min, k[~kept], texel_out[~kept])
    np.maximum.at(a_max, k[~kept], texel_out[~kept])
    seen = a_max >= 0
    if (a_min[seen] != a_max[seen]).any():
        bad = int(np.flatnonzero(seen & (a_min != a_max))[0])
        raise AliasStructureError("bin %d hands its draws to more than one other texel (%d and %d among them)" % (bad, a_min[bad], a_max[bad]))
    has_kept = np.zeros(n, bool)
    has_kept[k[kept]] = True
    crossed = seen & has_kept & ~(lo < hi)
    if crossed.any():
        bad = int(np.flatnonzero(crossed)[0])
        raise AliasStructureError("bin %d kept its texel at r2 = %.9g and gave it away at r2 = %.9g: no threshold separates them" % (bad, lo[bad], hi[bad]))
    a = np.where(seen, a_max, 0)
    unseen = float(((1.0 - lo[~seen])/n).sum())
    lower = lo/n
    upper = hi/n
    np.add.at(lower, a[seen], (1.0 - hi[seen])/n)
    np.add.at(upper, a[seen], (1.0 - lo[seen])/n)
    width = float((upper - lower).sum()) + unseen
    return lower, upper + unseen, width


def in_brackets(p, lower, upper):
    """Which p_i lie in [lower_i, upper_i], to the slack of what alias_structure takes as exact: a bin holds floor or ceil of 2^32/n of the
    first draw's values (n*2^-32 of its mass), and the threshold and r2 are float32 values on a 2^-24 grid (four such roundings: 2^-22);
    both relative to the bracket's end, plus 2^-32 absolute."""
    n = len(p)
    tol = (n*2.0**-32 + 2.0**-22)*upper + 2.0**-32
    return (p >= lower - tol) & (p <= upper + tol)



def alias_width_bound(rows, n):
    """What alias_structure's width may be for a sampler whose every bin has ONE threshold, at `rows` rows over n bins -- the cap where the
    row count is too small for a fixed one.  A bin with m rows leaves the interval of [0, 1] between the two r2 values next to its
    threshold undecided: each side is at most 1/(m + 1) long in expectation (m uniform points), 2/(m + 1) together; m is binomial(rows,
    1/n), so E[1/(m + 1)] = n/(rows + 1)*(1 - (1 - 1/n)^(rows + 1)); the width counts every interval twice, at 1/n each:
        E[width] <= 4*n/(rows + 1)*(1 - (1 - 1/n)^(rows + 1))        (1.469 at 200,000 rows over 80,000 bins)
    and as a sum over bins of terms in [0, 2/n] its standard deviation is at most 1/sqrt(n); six of them are added."""
    return 4.0*n/(rows + 1.0)*(1.0 - (1.0 - 1.0/n)**(rows + 1.0)) + 6.0/np.sqrt(n)


# ---------------------------------------------------------------------------
# what the host test and the GPU test share

W, H, PASSES = 48, 32, 4
SCENE = "features_probe"
LEAF_ROWS = 200_000
_ALIAS_ROWS = {"odd": 1_000_000, "flat": 1_000_000, "blackrows": 1_000_000}


def alias_rows(name):
    """how many seeds the alias arm's leaf is run on, in the model and on the GPU"""
    return _ALIAS_ROWS.get(name, LEAF_ROWS)


def alias_width_cap(name):
    """The cap on alias_structure's width: 1 % of the mass -- but on big, whose 200,000 rows are 2.5 a bin over 80,000 bins: no such row
    count brackets a threshold to 1 % (that takes some 400 rows a bin, 32,000,000 rows), so big is held to what its row count allows."""
    return alias_width_bound(alias_rows(name), probe(name).n) if name == "big" else 0.01


@functools.lru_cache(maxsize=None)
def pack(name):
    return lg.pack_bytes(name)


@functools.lru_cache(maxsize=None)
def blob(name):
    """features_probe.pack with the catalogue's probe `name`"""
    return with_probe(pack(SCENE), probe(name).texels)


@functools.lru_cache(maxsize=None)
def port_render(name, width=W, height=H, pass_begin=0, passes=PASSES, radiance=False):
    """the C restatement's render of features_probe with probe `name` (None: the pack's own): (accumulator, per-path radiance or None)"""
    b = pack(SCENE) if name is None else blob(name)
    cam, opt = lg.frame(b, width, height)
    O = oa.PortOracle()
    h = O.load_pack(b)
    try:
        acc, rad, _ = O.render_seeded(h, cam, opt, pass_begin, passes, threads=min(16, os.cpu_count() or 1), want_radiance=radiance)
    finally:
        O.free(h)
    acc.setflags(write=False)
    if rad is not None:
        rad.setflags(write=False)
    return acc, rad


@functools.lru_cache(maxsize=None)
def port_leaf(name, n):
    """port_leaf_probe of probe `name` on seeds(n)"""
    O = oa.PortOracle()
    h = O.load_pack(blob(name))
    try:
        out = O.probe(h, seeds(n))
    finally:
        O.free(h)
    for a in out:
        a.setflags(write=False)
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def model_rows(name, n, texel=None, factor=1.0):
    """(u1, r2, texels a float64 Vose table returns on seeds(n)); texel/factor: the table is built for probabilities with that one
    texel's scaled by `factor` and renormalised -- a wrong table, in the model only"""
    p = probe(name).p
    if texel is not None:
        p = p.copy()
        p[texel] *= factor
        p /= p.sum()
    keep, alias = vose(p)
    assert np.abs(table_probabilities(keep, alias) - p).max() < 2.0**-24       # keep is a float32: 2^-24 of 1/n per bin, n bins at most
    u1, r1, u2, r2 = draws(seeds(n))
    return u1, r2, alias_pick(keep, alias, u1, r2)


def frequencies_ok(p, texel_out, what):
    """per texel with D*p_i >= 50, the count within 6 binomial standard deviations of D*p_i; prints the worst"""
    D = len(texel_out)
    assert (texel_out >= 0).all()
    count = np.bincount(texel_out, minlength=len(p)).astype(np.float64)
    held = D*p >= 50
    z = np.abs(count - D*p)[held]/np.sqrt(D*p*(1.0 - p))[held] if held.any() and (p[held] < 1).all() else np.zeros(1)
    print("%s: %d texels with D*p >= 50, worst count %.2f standard deviations from D*p" % (what, int(held.sum()), float(z.max())))
    return bool((z <= 6.0).all()) and not (count[p == 0] > 0).any()


def mean_difference_z(a, b):
    """how many standard errors the mean of the per-pixel difference image (luminance of rgb/w) lies from 0, the error from the image itself"""
    def lum(x):
        w = np.where(x[..., 3:4] > 0, x[..., 3:4], 1.0)
        return (x[..., :3].astype(np.float64)/w).sum(axis=-1)/3.0
    d = (lum(a) - lum(b)).ravel()
    return float(abs(d.mean())/(d.std(ddof=1)/np.sqrt(d.size)))

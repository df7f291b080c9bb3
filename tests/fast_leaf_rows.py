"""The rows of the tolerance arm's leaf tables (tests/test_gpu_fast_leaf.py), host only: which materials, which input families, from which
seeds -- shared with tests/test_shade_f64.py, which pins the float64 statement to the reference on the same rows.

Materials are primitives of committed packs, chosen so that every class a BSDF branch depends on is present (CLASSES; asserted from the
packs' raw materials by test_shade_f64.test_the_materials_hold_every_class).  Three families of 65,536 rows per material:
  random       n, V, L uniform on the sphere, V turned above the surface, as test_gpu_leaf.test_bsdf_eval_pdf_sample
  grazing      n.V log-uniform in [1e-4, 1], n.L likewise with either sign: the Smith and Schlick terms' ends, 1/|n.L|
  near-mirror  L is V reflected about n, then turned by an angle log-uniform in [1e-5, 1e-1] rad about a random axis: where GTR2 peaks
               and the max(1e-6, L.H) guard lives
with the index pair (etaI, etaO) drawn from (1, 1.5), (1.5, 1), (1, 1) on every row -- in the grazing family from the first two only: with
equal indices Fr computes LDotN = sqrt(1 - (1 - (n.V)^2)), and below n.V = 1e-3 that difference is within 1e-6 of the `SinThetaT2 > 1`
comparison and within a few float32 roundings of 0 -- a quarter of the family's rows would be rows no arithmetic owns.  That corner is
held by class in the edge rows of test_gpu_fast_leaf (etaI == etaO at n.V = 1e-3, 1e-7 and 0).
"""
import functools

import numpy as np

import tinsel_amd
from tests import shade_f64 as s64
from tests.test_gpu_ray_query import _pack

N = 65536
FAMILIES = ("random", "grazing", "near-mirror")
ETA_PAIRS = np.array([[1.0, 1.5], [1.5, 1.0], [1.0, 1.0]], np.float32)
CLASSES = ("transmission=0", "0<transmission<1", "transmission=1", "subsurface>0", "clearcoat>0,alpha<1", "metallic>0", "roughness<=0.001",
           "roughness>=0.5")
# (pack, primitive): what the material brings
MATERIALS = (
    ("features", 0),    # clearcoat 0.7 (alpha 0.06), roughness 0.6, specular 0.3
    ("features", 4),    # transmission 0.85, roughness 0.05
    ("features", 5),    # subsurface 0.6
    ("features", 7),    # transmission 0.6, metallic 0.2
    ("cornell", 7),     # metallic 1, roughness 0.1
    ("glass", 7),       # transmission 0.9, roughness 0.005: the glass scene's own
    ("veach", 2),       # metallic 0.9, roughness 0.05: the veach scene's plates
    ("gloss", 0),       # metallic 0.9, roughness 0.01
    ("fuzz:00", 0),     # roughness at the 0.001 floor, metallic 0.42, specular tint 0.45
    ("fuzz:00", 10),    # transmission 1, roughness 0.71
    ("fuzz:02", 0),     # transmission 1, roughness 0.02
    ("fuzz:06", 1),     # transmission 0.9 with roughness at the floor
    ("fuzz:01", 6),     # subsurface 0.72 with roughness at the floor, metallic 0.74
    ("fuzz:07", 5),     # clearcoat 0.84 (alpha 0.08), roughness 0.02, specular tint 0.83
)
# PrimitiveSample: emitters of both samplable types, a moving one among them
LIGHTS = (("features", 2), ("features", 3), ("cornell", 5), ("veach", 5), ("fuzz:00", 8), ("fuzz:03", 8))
SCENES = tuple(dict.fromkeys(s for s, _ in MATERIALS + LIGHTS))
# Every seed (all 2^32 were scanned) whose SECOND Randf() is exactly 1.0f: the draw is 2^32 - 128 or more and rounds up to 2^32.  On the BRDF
# branch that draw is r1 of Sample2D (disney.h:241), and CosineSampleHemisphere(1, r2) takes z = sqrt(Max(0, 1 - cos^2 - sin^2)) of a
# difference that is a rounding error of either sign: the rows on which the Max(0, .) is all that stands between z and NaN.  Random rows
# meet one such draw in 3e7.
R1_ONE_SEEDS = (
    32418902, 65966622, 95789306, 110558804, 220241688, 379624053, 410227903, 452831547, 503947688, 529179598, 540457456, 563734558,
    578772409, 637446413, 696973563, 833712763, 857239479, 943672648, 956384985, 996910696, 998166430, 1036214779, 1040270216,
    1061810786, 1068216915, 1117678643, 1119929330, 1144001551, 1225606688, 1244226390, 1334313137, 1460719523, 1479834799,
    1496034359, 1610270486, 1616560476, 1704203237, 1769974089, 1813242092, 1833036858, 1896852082, 2006740138, 2055932445,
    2070056318, 2163679485, 2164219209, 2350914698, 2366683476, 2387940390, 2485848682, 2494288158, 2495112118, 2518125297,
    2528930521, 2561474045, 2626948832, 2640477833, 2640544233, 2650273967, 2662388817, 2688785879, 2702661982, 2726403188,
    2788997886, 2847244557, 2892469227, 2927817463, 2951565202, 2996527582, 3030969371, 3109638497, 3136895617, 3137655047,
    3213493505, 3231182788, 3247641956, 3309781346, 3390713717, 3399695449, 3459675448, 3472451117, 3481544385, 3488150407,
    3535594615, 3583175789, 3590160254, 3596917259, 3681819391, 3705782558, 3736186960, 3816588422, 3820034107, 3852680454,
    3889944559, 3979163680, 4072055494, 4188345474, 4216045498, 4232068521, 4251195369, 4256219057,
)


@functools.lru_cache(maxsize=None)
def scene(name):
    return tinsel_amd.Scene(_pack(name))


@functools.lru_cache(maxsize=None)
def material(name, prim):
    return s64.materials(scene(name))[prim]


def _unit(v):
    return v/np.linalg.norm(v, axis=1, keepdims=True)


def _tangent(rng, w):
    """a random unit vector perpendicular to the unit vectors w [n, 3]"""
    t = rng.normal(size=w.shape)
    t -= (t*w).sum(axis=1, keepdims=True)*w
    return _unit(t)


def _log_uniform(rng, n, lo, hi):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), size=n))


def _seed(family, name, prim):
    return [20261021, FAMILIES.index(family), MATERIALS.index((name, prim))]


@functools.lru_cache(maxsize=None)
def eval_rows(family, name, prim):
    """rows [N, 11] float32 for BSDFEval / BSDFPdf (op 2): n(3) V(3) L(3) etaI etaO.  Read-only, shared"""
    rng = np.random.default_rng(_seed(family, name, prim))
    n = _unit(rng.normal(size=(N, 3)))
    if family == "random":
        V, L = _unit(rng.normal(size=(N, 3))), _unit(rng.normal(size=(N, 3)))
        V = np.where((V*n).sum(axis=1, keepdims=True) < 0, -V, V)
    elif family == "grazing":
        cv, cl = _log_uniform(rng, N, 1e-4, 1.0), _log_uniform(rng, N, 1e-4, 1.0)*rng.choice([-1.0, 1.0], size=N)
        V = cv[:, None]*n + np.sqrt(1.0 - cv*cv)[:, None]*_tangent(rng, n)
        L = cl[:, None]*n + np.sqrt(1.0 - cl*cl)[:, None]*_tangent(rng, n)
    else:
        V = _unit(rng.normal(size=(N, 3)))
        V = np.where((V*n).sum(axis=1, keepdims=True) < 0, -V, V)
        R = 2.0*(V*n).sum(axis=1, keepdims=True)*n - V
        ang = _log_uniform(rng, N, 1e-5, 1e-1)
        L = np.cos(ang)[:, None]*R + np.sin(ang)[:, None]*_tangent(rng, R)
    eta = ETA_PAIRS[rng.integers(0, 2 if family == "grazing" else len(ETA_PAIRS), size=N)]
    rows = np.ascontiguousarray(np.concatenate([n, V, L, eta], axis=1).astype(np.float32))
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def sample_rows(family, name, prim):
    """(rows [N, 8] float32: n(3) V(3) etaI etaO, seeds [N] uint32) for BSDFSample (op 3): the eval rows' n, V and indices"""
    r = eval_rows(family, name, prim)
    rows = np.ascontiguousarray(np.concatenate([r[:, 0:6], r[:, 9:11]], axis=1))
    seeds = np.random.default_rng(_seed(family, name, prim) + [3]).integers(0, 2**32, size=N, dtype=np.uint64).astype(np.uint32)
    rows.setflags(write=False)
    seeds.setflags(write=False)
    return rows, seeds


@functools.lru_cache(maxsize=None)
def r1_one_rows():
    """(rows [k, 8] float32, seeds [k] uint32) for BSDFSample: every seed of R1_ONE_SEEDS under 16 random normals and views, indices 1 -> 1"""
    rng = np.random.default_rng([20261021, 8])
    k = 16*len(R1_ONE_SEEDS)
    n, V = _unit(rng.normal(size=(k, 3))), _unit(rng.normal(size=(k, 3)))
    V = np.where((V*n).sum(axis=1, keepdims=True) < 0, -V, V)
    rows = np.ascontiguousarray(np.concatenate([n, V, np.ones((k, 2))], axis=1).astype(np.float32))
    seeds = np.repeat(np.array(R1_ONE_SEEDS, np.uint32), 16)
    rows.setflags(write=False)
    seeds.setflags(write=False)
    return rows, seeds


def camera_rows():
    """raster points [N, 2] float32 of a 1920 x 1080 frame for GenerateRay (op 1)"""
    return (np.random.default_rng([20261021, 1]).random((N, 2))*[1920, 1080]).astype(np.float32)


def probe_seeds():
    """seeds [N] uint32 for ProbeSample (op 6); tests/golden/make_fast_leaf_yardstick.py records the reference's two builds on the same"""
    return np.random.default_rng([20261021, 6]).integers(0, 2**32, size=N, dtype=np.uint64).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def light_rows(name, prim):
    """(times [N, 1] float32, seeds [N] uint32) for PrimitiveSample (op 5)"""
    rng = np.random.default_rng([20261021, 5, LIGHTS.index((name, prim))])
    times = rng.random((N, 1)).astype(np.float32)
    seeds = rng.integers(0, 2**32, size=N, dtype=np.uint64).astype(np.uint32)
    times.setflags(write=False)
    seeds.setflags(write=False)
    return times, seeds

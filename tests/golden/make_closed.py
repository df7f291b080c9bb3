#!/usr/bin/env python3
"""Closed-set parity corpus: tests/golden/closed.golden.npz.

Six small scenes that the batch plan gives the CLOSED FIT instance of k_bounce (and with it a baked instance: tn_baked.h) when regions are
not shared, each built around a part of those two kernels that cornell never runs: light tables of 2, 4 (baked::kLightSelectMax) and 5
lights with different sample counts, sphere lights, no light at all, no plane table, a plane table of sixteen slots, a ninth slot after the
pair block, primitives 62 and 63 of the scan mask, and everywhere random unit quaternions, non-dyadic scales and radii, and a 37 x 29 frame
(3 passes: 3219 paths, no multiple of 64).  The scenes are written as .tin text from a seed, loaded by the reference's own loader +
Scene::Build and rendered by its PathTrace under the per-path seed contract; the file keeps, per scene, the pack's bytes, the per-path
radiance, the accumulator, the first pass and a table of expected facts (primitives, plane-table slots, the pair blocks' end, lights, light
samples, the scan mask) -- taken from the scene AS WRITTEN HERE by this file's own statement of the plane-table rule (`facts`), not from the
library's generated header, which tests/test_closed_corpus.py holds against them.  Needs /root/reference and a built library.

The rule that decides which scenes are closed (tn_host_batch.h plans_fit_closed, fit_bounce, bounce_features; tn_host_create.h
set_scene_flags): the closed instance is compiled for the feature set {spheres} alone, so a slim scene (no medium, probe, motion, walked
mesh, transmission or subsurface) with at most one mesh primitive (two defer their walks: the deferred instance) gets it only where neither
kFeatPools nor kFeatSort is asked for.  Pools are planned for every scene that is not ENCLOSED (plan_bounce: `!sceneEnclosed`), and a scene
is enclosed where two of its planes have opposing normals (cosine below -0.99: a floor and a ceiling); the queue sort is planned for scenes
with at most two always-hit planes.  So: an opposing plane pair, and at least three planes.  Three walls of an open corner are refused
("the scene's features lie outside the closed FIT set": tests/test_bake_source.py has that scene); a floor, a ceiling and a wall are taken.
No ray leaves such a scene but along the pair, so the sky lights nothing here: every scene has an emitter.

The generator refuses to write the file unless every scene is slim, has feature bits 16 (spheres), is bakeable under
abi.Tuning(bounce_share=0), has finite radiance and light on at least half of its paths.  A scene that fails gets another seed or
placement below, never a lower bar.

Usage:  python tests/golden/make_closed.py            (deterministic: the same bytes every time)"""
import io
import os
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests.oracle_api import RefOracle  # noqa: E402

WIDTH, HEIGHT, PASSES = 37, 29, 3
OUT = os.path.join(HERE, "closed.golden.npz")

# name -> seed (the random stream of everything the scene draws)
SCENES = {
    "two-lights": 1,
    "four-sphere-lights": 2,
    "five-lights": 3,
    "no-light": 9,
    "sixty-four": 11,
    "thirteen-planes": 6,
}
FACTS = ("prims", "planes", "pair_end", "lights", "samples")

QUAD = """mesh quad
{
	verts 4
	-0.5 0 0.5
	0.5 0 0.5
	0.5 0 -0.5
	-0.5 0 -0.5

	tris 2
	0 2 1
	0 3 2
}"""

# cornell's box: floor, two side walls, ceiling, back wall; open towards the camera
WALLS = [(0.0, 1.0, 0.0, 0.0), (1.0, 0.0, 0.0, 1.0), (-1.0, 0.0, 0.0, 1.0), (0.0, -1.0, 0.0, 2.0), (0.0, 0.0, 1.0, 1.0)]


def fmt(v):
    return " ".join("%.6g" % float(x) for x in np.atleast_1d(v))


def unit(v):
    v = np.asarray(v, np.float64)
    return v/np.linalg.norm(v)


def material(rng, name, emitter=False):
    """roughness, specular, metallic, clearcoat, sheen and specularTint over their ranges; never transmission, absorption or subsurface"""
    lines = ["material %s" % name, "{"]
    if emitter:
        lines.append("\temission %s" % fmt(rng.uniform(4.0, 25.0, 3)))
        lines.append("\tcolor %s" % fmt(rng.uniform(0.0, 0.6, 3)*(rng.random() < 0.5)))
    else:
        lines.append("\tcolor %s" % fmt(rng.uniform(0.3, 0.95, 3)))
    lines.append("\troughness %s" % fmt(rng.choice([0.02, 0.1, 0.3, 0.6, 1.0]) if rng.random() < 0.5 else rng.uniform(0.0, 1.0)))
    lines.append("\tspecular %s" % fmt(rng.uniform(0.0, 1.0)))
    lines.append("\tmetallic %s" % fmt(rng.choice([0.0, 0.0, 1.0, rng.uniform(0, 1)])))
    if rng.random() < 0.4:
        lines.append("\tclearcoat %s" % fmt(rng.uniform(0.1, 1.0)))
        lines.append("\tclearcoatGloss %s" % fmt(rng.uniform(0.0, 1.0)))
    if rng.random() < 0.4:
        lines.append("\tsheen %s" % fmt(rng.uniform(0, 1)))
    if rng.random() < 0.4:
        lines.append("\tspecularTint %s" % fmt(rng.uniform(0, 1)))
    lines.append("}")
    return "\n".join(lines)


class Builder:
    """a scene as a list of primitives (dicts: kind, the text's own numbers, light samples), its materials, and the .tin text of both"""

    def __init__(self, name, seed):
        self.name, self.rng = name, np.random.default_rng(7000 + seed)
        self.prims, self.mats = [], []
        self.camera = "0 1 4"               # cornell's, looking down -z
        self.depth = int(self.rng.integers(3, 8))
        self.filter = "%s %s %s" % (self.rng.choice(["gaussian", "box"]), fmt(self.rng.choice([0.75, 1.0, 1.5, 2.0])), fmt(self.rng.uniform(0.5, 3.0)))
        for _ in range(4):
            self.mat()

    def mat(self, emitter=False):
        name = "%s%d" % ("e" if emitter else "m", len(self.mats))
        self.mats.append(material(self.rng, name, emitter))
        return name

    def any_mat(self):
        return "m%d" % int(self.rng.integers(0, 4))

    def pose(self, lo, hi, scale=(0.4, 1.7)):
        q = self.rng.normal(size=4)
        return ["\tposition %s" % fmt(self.rng.uniform(lo, hi)), "\trotation %s" % fmt(q/np.linalg.norm(q)), "\tscale %s" % fmt(self.rng.uniform(*scale))]

    def plane(self, eq, mat=None):
        # the equation as the text states it (nine digits: a float32 by its value), so that `facts` pairs what the loader will read
        text = ["%.9g" % float(np.float32(c)) for c in eq]
        self.prims.append({"kind": "plane", "eq": tuple(np.float32(t) for t in text), "samples": 0,
                           "text": ["\ttype plane", "\tplane %s" % " ".join(text), "\tmaterial %s" % (mat or self.any_mat())]})

    def sphere(self, samples=0, emissive=False, lo=(-0.7, 0.3, -0.7), hi=(0.7, 1.7, 0.7), radius=(0.05, 0.3), scale=(0.4, 1.7)):
        mat = self.mat(True) if (samples or emissive) else self.any_mat()
        text = ["\ttype sphere"] + self.pose(lo, hi, scale) + ["\tradius %s" % fmt(self.rng.uniform(*radius)), "\tmaterial %s" % mat]
        self.prims.append({"kind": "sphere", "samples": samples, "text": text + (["\tlightSamples %d" % samples] if samples else [])})

    def quad(self, samples=0, lo=(-0.5, 1.2, -0.5), hi=(0.5, 1.8, 0.5)):
        mat = self.mat(True) if samples else self.any_mat()
        text = ["\ttype mesh", "\tmesh quad"] + self.pose(lo, hi) + ["\tmaterial %s" % mat]
        self.prims.append({"kind": "mesh", "samples": samples, "text": text + (["\tlightSamples %d" % samples] if samples else [])})

    def walls(self):
        for eq in WALLS:
            self.plane(eq)

    def text(self):
        out = ["# closed-set scene: %s" % self.name, "options", "{", "\twidth %d" % WIDTH, "\theight %d" % HEIGHT, "\tmaxDepth %d" % self.depth,
               "\tfilter %s" % self.filter, "}", "", "camera", "{", "\tposition %s" % self.camera, "\trotation 0 0 0 1", "\tfov 35", "}", ""]
        out += self.mats + [QUAD]
        out += ["\n".join(["primitive", "{"] + p["text"] + ["}"]) for p in self.prims]
        return "\n\n".join(out) + "\n"


def two_lights(b):
    b.walls()
    b.quad(samples=2)
    b.sphere(samples=3)
    for _ in range(3):
        b.sphere()


def four_sphere_lights(b):
    n = unit([0.12, 1.0, 0.08])
    planes = [tuple(n) + (0.0,), (1.0, 0.0, 0.0, 1.2), tuple(-n) + (2.4,), (0.0, 0.0, 1.0, 1.2)]
    for samples, eq in zip((1, 3, 2, 1), planes):
        b.sphere(samples=samples, lo=(-0.7, 0.5, -0.7))
        b.plane(eq)


def five_lights(b):
    b.walls()
    for samples in (2, 1, 3, 1):
        b.sphere(samples=samples)
    b.quad(samples=1)
    for _ in range(2):
        b.sphere()


CEILING = 1.2          # (no-light's)


def no_light(b):
    for eq in (WALLS[0], (0.0, -1.0, 0.0, CEILING), WALLS[4]):
        b.plane(eq)
    b.camera = "0 0.6 1.7"              # (close by: a path finds the emitter by itself or not at all, and from cornell's distance one in six does)
    b.sphere(lo=(-0.7, 0.2, -0.7), hi=(0.7, CEILING - 0.2, 0.7))
    # emission without lightSamples: found by BSDF rays only, so the largest sphere the ranges allow, in the middle of a low room
    b.sphere(emissive=True, lo=(-0.3, 0.5, -0.3), hi=(0.3, CEILING - 0.5, 0.3), radius=(0.28, 0.3), scale=(1.5, 1.7))
    b.sphere(lo=(-0.7, 0.2, -0.7), hi=(0.7, CEILING - 0.2, 0.7))
    b.quad(lo=(-0.6, 0.3, -0.5), hi=(0.6, CEILING - 0.3, 0.5))


def sixty_four(b):
    b.walls()
    for _ in range(57):
        b.sphere(lo=(-0.9, 0.1, -0.9), hi=(0.9, 1.5, 0.9))
    b.quad(samples=1, lo=(-0.3, 1.7, -0.3), hi=(0.3, 1.9, 0.3))
    b.sphere(samples=1, lo=(-0.5, 1.6, 0.2), hi=(0.5, 1.8, 0.8))


def thirteen_planes(b):
    b.walls()
    for _ in range(8):
        b.plane(tuple(unit(b.rng.normal(size=3))) + (float(b.rng.uniform(6.0, 9.0)),))
    b.quad(samples=1)
    b.sphere(samples=2)


MAKERS = {"two-lights": two_lights, "four-sphere-lights": four_sphere_lights, "five-lights": five_lights, "no-light": no_light,
          "sixty-four": sixty_four, "thirteen-planes": thirteen_planes}


def build(name):
    b = Builder(name, SCENES[name])
    MAKERS[name](b)
    return b


def _opposing(a, b):
    """two plane equations the table tests as a pair: every normal component of b the negation of a's by its bits, or both zero"""
    for x, y in zip(a[:3], b[:3]):
        if np.float32(y).view(np.uint32) != (np.float32(x).view(np.uint32) ^ np.uint32(0x80000000)) and not (x == 0.0 and y == 0.0):
            return False
    return all(np.isfinite(a)) and all(np.isfinite(b))


def facts(prims):
    """(primitives, plane-table slots in use, end of the pair blocks, lights, light samples), scan mask -- from the primitive list alone.  The
    table exists from four planes up; opposing planes pair greedily in list order; a block of eight slots holds two pairs and one single plane
    (A0 B0 A1 B1 R - - -), the singles left follow one per slot; the scan visits what is not in the table"""
    planes = [k for k, p in enumerate(prims) if p["kind"] == "plane"]
    lights = [p["samples"] for p in prims if p["samples"] > 0]
    slots, pair_end, mask = 0, 0, (1 << len(prims)) - 1
    if len(planes) >= 4:
        used, pairs = set(), 0
        for i, a in enumerate(planes):
            for c in planes[i + 1:]:
                if a not in used and c not in used and _opposing(prims[a]["eq"], prims[c]["eq"]):
                    used |= {a, c}
                    pairs += 1
        singles, blocks = len(planes) - 2*pairs, (pairs + 1)//2
        pair_end = 8*blocks
        slots = pair_end + singles - min(blocks, singles)
        for k in planes:
            mask &= ~(1 << k)
    return (len(prims), slots, pair_end, len(lights), sum(lights)), mask


def _write_npz(path, arrays):
    """np.savez_compressed's format with the zip's time stamps fixed: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    import tinsel_amd
    from tinsel_amd import abi
    R = RefOracle()
    d = tempfile.mkdtemp()
    out = {"names": np.array(list(SCENES)), "fact_names": np.array(FACTS), "passes": np.int32(PASSES)}
    for k, name in enumerate(SCENES):
        b = build(name)
        tin = os.path.join(d, "closed%d.tin" % k)
        with open(tin, "w") as f:
            f.write(b.text())
        h = R.load_tin(tin)
        assert R.num_primitives(h) == len(b.prims), name
        pack = os.path.join(d, "closed%d.pack" % k)
        R.write_pack(h, pack)
        cam, opt = R.camera_options(h)
        assert (opt.width, opt.height, opt.max_depth) == (WIDTH, HEIGHT, b.depth), name
        first = 5*k
        accum, rad, _ = R.render_seeded(h, cam, opt, first, PASSES, want_accum=True, want_radiance=True, threads=8)
        R.free(h)
        with open(pack, "rb") as f:
            blob = f.read()
        scene = tinsel_amd.Scene(blob)
        _, _, ok, why = scene.bake_source(abi.Tuning(bounce_share=0))
        lit = float(rad.any(axis=-1).mean())
        row, mask = facts(b.prims)
        print("%-20s seed %d depth %d prims %2d table %2d/%d lights %d (%d samples) pack %.1f KB lit %.1f %% mean %.4f" % (
            name, SCENES[name], b.depth, row[0], row[1], row[2], row[3], row[4], len(blob)/1e3, 100*lit, float(rad.mean())))
        assert scene.bounce_slim() and scene.bounce_features() == abi.BOUNCE_SPHERE, (name, scene.bounce_features())
        assert ok, (name, why)
        assert np.isfinite(rad).all() and np.isfinite(accum).all(), name
        assert lit >= 0.5, "%s: light on %.1f %% of the paths only" % (name, 100*lit)
        out["pack_%d" % k] = np.frombuffer(blob, np.uint8)
        out["radiance_%d" % k] = rad
        out["accum_%d" % k] = accum
        out["first_pass_%d" % k] = np.int32(first)
        out["facts_%d" % k] = np.array(row, np.int64)
        out["scan_mask_%d" % k] = np.uint64(mask)
    _write_npz(OUT, out)
    print("wrote closed.golden.npz (%.1f KB)" % (os.path.getsize(OUT)/1e3))
    assert os.path.getsize(OUT) < 1000000


if __name__ == "__main__":
    main()

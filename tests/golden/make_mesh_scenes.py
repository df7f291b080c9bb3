#!/usr/bin/env python3
"""Seeded mesh-heavy scenes: .tin text with the meshes inline, for the reference's own loader + Scene::Build (RefOracle.load_tin / write_pack).

The fuzz generator (make_fuzz.py) knows three meshes of 2, 4 and 8 triangles; here the meshes are procedural, a function of (shape, n, seed),
n from 9 to 20,000 triangles:
    soup    n loose triangles in clusters of very different sizes and densities (an unbalanced SAH tree)
    sheet   a wavy height field of n triangles over shared vertices
    sphere  a closed, dented UV sphere of about n triangles
    torus   a closed torus of about n triangles
every one inside the unit ball, so that a primitive's `scale` is its radius.  Materials and poses are make_fuzz's (material, pose); the camera stands
still at a fixed position and looks at the origin, the primitives are laid out in a grid of cells facing it.

Families (each a function of a seed; 320 x 240, maxDepth drawn from {3, 4, 6}) and what they are for -- tests/test_gpu_mesh_scenes.py:
    one_big      one mesh of about 20,000 triangles, spheres, planes, a sphere light
    seven        exactly seven mesh primitives of 500 ... 5,000 triangles, at least two light samples
    twelve       twelve mesh primitives of 9 ... 5,000 triangles: more than the seven the walk kernel takes
    instances    sixteen primitives of two meshes, each with its own pose, every third moving and turning during the shutter
    mesh_light   the emitter is a closed mesh of 2,000 triangles or more with 2-3 light samples
    beyond_flat  70 ... 100 primitives (spheres, up to 7 planes), 3 ... 10 of them meshes of 500 triangles or more

Usage:  python tests/golden/make_mesh_scenes.py FAMILY SEED > scene.tin"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests.golden.make_fuzz import f3, material, pose  # noqa: E402

F = np.float32
FAMILIES = ("one_big", "seven", "twelve", "instances", "mesh_light", "beyond_flat")
WIDTH, HEIGHT = 320, 240
CAMERA = ((0.0, 0.5, 9.0), (0.0, 0.0, 0.0), 40.0)          # position, target, fov
MAX_LIGHTS, MAX_LIGHT_SAMPLES = 3, 3                        # the most shadow rays per bounce a scene can ask for: 9


# ---------------------------------------------------------------------------------------------------------------------------------
# meshes: (positions [V,3] float32, indices [n,3] int32) inside the unit ball

def _fit(pos):
    pos = pos - 0.5*(pos.min(axis=0) + pos.max(axis=0))
    return (pos/np.linalg.norm(pos, axis=1).max()).astype(F)


def _soup(rng, n):
    """clusters of 1/2, 1/4, 1/8 ... of the triangles, each a tenth to the whole of the mesh wide, triangle sizes over a decade and a half"""
    share = 0.5**np.arange(1, 9)
    which = rng.choice(len(share), n, p=share/share.sum())
    centre = rng.uniform(-0.7, 0.7, (len(share), 3))
    width = 10.0**rng.uniform(-1.0, 0.0, len(share))*0.5
    c = centre[which] + rng.normal(size=(n, 3))*width[which, None]*0.5
    size = 10.0**rng.uniform(-1.5, 0.0, (n, 1, 1))*0.25
    t = c[:, None, :] + rng.uniform(-1.0, 1.0, (n, 3, 3))*size
    return _fit(t.reshape(-1, 3)), np.arange(3*n, dtype=np.int32).reshape(n, 3)


def _quads(w, h, wrap_x, wrap_y):
    """two triangles per cell of a w x h grid of vertices numbered j*w + i"""
    idx = []
    for j in range(h if wrap_y else h - 1):
        for i in range(w if wrap_x else w - 1):
            a, b = j*w + i, j*w + (i + 1) % w
            c, d = ((j + 1) % h)*w + (i + 1) % w, ((j + 1) % h)*w + i
            idx += [(a, b, c), (a, c, d)]
    return idx


def _sheet(rng, n):
    q = (n + 1)//2
    w = max(1, int(np.ceil(np.sqrt(q))))
    h = (q + w - 1)//w
    x, y = np.meshgrid(np.linspace(-1.0, 1.0, w + 1), np.linspace(-1.0, 1.0, h + 1))
    k, ph = rng.uniform(1.0, 5.0, 4), rng.uniform(0.0, 6.28, 4)
    z = 0.25*np.sin(k[0]*x + ph[0])*np.cos(k[1]*y + ph[1]) + 0.1*np.sin(k[2]*(x + y) + ph[2]) + 0.02*rng.normal(size=x.shape)
    pos = np.stack([x.ravel(), y.ravel(), z.ravel()], 1)
    return _fit(pos), np.array(_quads(w + 1, h + 1, False, False)[:n], np.int32)


def _sphere(rng, n):
    """slices x stacks, the poles single vertices: 2*slices*(stacks - 1) triangles, the largest number not above n (at least 3 x 2)"""
    stacks = max(2, int(round(np.sqrt(n/4.0))) + 1)
    slices = max(3, n//(2*(stacks - 1)))
    k, ph = rng.integers(1, 5, 3), rng.uniform(0.0, 6.28, 3)
    th = np.pi*np.arange(1, stacks)/stacks
    lo = 2.0*np.pi*np.arange(slices)/slices
    T, L = np.meshgrid(th, lo, indexing="ij")
    rad = 1.0 + 0.12*np.sin(k[0]*T + ph[0])*np.cos(k[1]*L + ph[1]) + 0.05*np.sin(k[2]*L + ph[2])
    ring = np.stack([rad*np.sin(T)*np.cos(L), rad*np.cos(T), rad*np.sin(T)*np.sin(L)], -1).reshape(-1, 3)
    pos = np.concatenate([ring, [[0.0, 1.0, 0.0], [0.0, -1.0, 0.0]]])
    top, bottom = len(ring), len(ring) + 1
    idx = _quads(slices, stacks - 1, True, False)
    last = (stacks - 2)*slices
    for i in range(slices):
        idx.append((top, (i + 1) % slices, i))
        idx.append((bottom, last + i, last + (i + 1) % slices))
    return _fit(pos), np.array(idx, np.int32)


def _torus(rng, n):
    """a x b quads around the two circles: 2ab triangles, the largest number not above n (at least 3 x 3)"""
    b = max(3, int(round(np.sqrt(n/6.0))))
    a = max(3, n//(2*b))
    minor = float(rng.uniform(0.2, 0.45))
    U, V = np.meshgrid(2.0*np.pi*np.arange(a)/a, 2.0*np.pi*np.arange(b)/b)       # (b rows of a vertices)
    pos = np.stack([(1.0 + minor*np.cos(V))*np.cos(U), minor*np.sin(V), (1.0 + minor*np.cos(V))*np.sin(U)], -1).reshape(-1, 3)
    return _fit(pos), np.array(_quads(a, b, True, True), np.int32)


SHAPES = {"soup": _soup, "sheet": _sheet, "sphere": _sphere, "torus": _torus}
CLOSED = ("sphere", "torus")


def make_mesh(shape, n, seed=0):
    rng = np.random.default_rng([n, seed, sum(map(ord, shape))])
    pos, idx = SHAPES[shape](rng, int(n))
    assert len(idx) >= 1 and idx.min() >= 0 and idx.max() < len(pos)
    return np.ascontiguousarray(pos, F), np.ascontiguousarray(idx, np.int32)


def mesh_text(name, pos, idx):
    vt = "\n".join("\t%.9g %.9g %.9g" % tuple(p) for p in pos.astype(np.float64))
    tt = "\n".join("\t%d %d %d" % tuple(t) for t in idx)
    return "mesh %s\n{\n\tverts %d\n%s\n\n\ttris %d\n%s\n}" % (name, len(pos), vt, len(idx), tt)


# ---------------------------------------------------------------------------------------------------------------------------------
# scenes

def _block(kind, lines, mat, light_samples=0):
    out = ["primitive", "{", "\ttype %s" % kind] + lines + ["\tmaterial %s" % mat]
    if light_samples:
        out.append("\tlightSamples %d" % light_samples)
    return "\n".join(out + ["}"])


def _cells(rng, count):
    """centres and radius of `count` cells of a grid that fills the camera's view of the plane z = 0, in a drawn order"""
    cols = int(np.ceil(np.sqrt(count*4.0/3.0)))
    rows = (count + cols - 1)//cols
    w, h = 8.4/cols, 6.0/rows
    centres = [((i + 0.5)*w - 4.2, (j + 0.5)*h - 3.0, 0.0) for j in range(rows) for i in range(cols)]
    order = rng.permutation(len(centres))[:count]
    return [centres[k] for k in order], 0.8*min(w, h)


class _Scene:
    def __init__(self, family, seed):
        self.rng = rng = np.random.default_rng([seed, FAMILIES.index(family), 77])
        self.family, self.seed = family, seed
        self.head = ["# %s %d" % (family, seed), "options", "{", "\twidth %d" % WIDTH, "\theight %d" % HEIGHT,
                     "\tmaxDepth %d" % int(rng.choice([3, 4, 6])),
                     "\tfilter %s %.6g %.6g" % (rng.choice(["gaussian", "box"]), float(rng.choice([0.5, 0.75, 1.0, 1.5, 2.0])), float(rng.uniform(0.5, 3.0)))]
        if rng.random() < 0.3:
            self.head.append("\tclamp %.6g" % float(rng.uniform(2.0, 8.0)))
        a = float(rng.uniform(0.0, 0.3))
        self.head += ["}", "", "camera", "{", "\tposition %s" % f3(CAMERA[0]), "\ttarget %s" % f3(CAMERA[1]), "\tfov %.6g" % CAMERA[2],
                      "\tshutterstart %.6g" % a, "\tshutterend %.6g" % (a + float(rng.uniform(0.2, 0.7))), "}", "",
                      "sky", "{", "\thorizon %s" % f3(rng.uniform(0.2, 1.0, 3)), "\tzenith %s" % f3(rng.uniform(0.2, 1.0, 3)), "}", ""]
        self.nmat = int(rng.integers(3, 7))
        self.materials = [material(rng, "m%d" % m, False) for m in range(self.nmat)]
        self.meshes, self.prims = [], []

    def mat(self):
        return "m%d" % int(self.rng.integers(0, self.nmat))

    def mesh(self, shape, n):
        name = "g%d" % len(self.meshes)
        self.meshes.append(mesh_text(name, *make_mesh(shape, n, 1000*self.seed + len(self.meshes))))
        return name

    def place(self, name, centre, radius, mat=None, moving=None, light_samples=0):
        moving = bool(self.rng.random() < 0.25) if moving is None else moving
        lines = pose(self.rng, centre=centre, spread=0.12*radius, scale=(0.85*radius, radius), moving=moving)
        self.prims.append(_block("mesh", lines + ["\tmesh %s" % name], mat or self.mat(), light_samples))

    def sphere(self, centre, spread, radius, mat=None, light_samples=0):
        lines = pose(self.rng, centre=centre, spread=spread, scale=(1.0, 1.0), moving=bool(self.rng.random() < 0.2))
        self.prims.append(_block("sphere", lines + ["\tradius %.6g" % float(self.rng.uniform(*radius))], mat or self.mat(), light_samples))

    def plane(self, which):
        n, d = [((0, 1, 0), 3.4), ((0, 0, 1), 5.0), ((1, 0, 0), 6.0), ((-1, 0, 0), 6.0), ((0, -1, 0), 6.0), ((0, 0.6, 0.8), 6.5), ((0.6, 0, 0.8), 7.0)][which]
        self.prims.append(_block("plane", ["\tplane %s %.6g" % (f3(n), d + float(self.rng.uniform(0.0, 0.5)))], self.mat()))

    def sphere_lights(self, count, samples):
        """`count` sphere lights above and in front of the grid; samples: a number for each, or None: 1-3 drawn"""
        for k in range(count):
            name = "e%d" % k
            self.materials.append(material(self.rng, name, True))
            centre = (float(self.rng.uniform(-3.0, 3.0)), float(self.rng.uniform(2.6, 3.6)), float(self.rng.uniform(2.0, 5.0)))
            self.sphere(centre, 0.0, (0.3, 0.8), mat=name, light_samples=samples if samples else int(self.rng.integers(1, MAX_LIGHT_SAMPLES + 1)))

    def shapes(self, count):
        """a shape per mesh, at least one of them a soup"""
        s = [str(self.rng.choice(["soup", "sheet", "sphere", "torus"])) for _ in range(count)]
        s[int(self.rng.integers(0, count))] = "soup"
        return s

    def text(self):
        return "\n\n".join(["\n".join(self.head)] + self.materials + self.meshes + self.prims) + "\n"


def scene_text(family, seed, most_lights=False):
    """most_lights (family seven): MAX_LIGHTS lights of MAX_LIGHT_SAMPLES samples each -- the most shadow rays per bounce the generator gives"""
    s = _Scene(family, seed)
    rng = s.rng
    if family == "one_big":
        shape = ["soup", "sphere", "torus", "sheet"][seed % 4]
        # (a soup is mostly gaps: it is made larger than the frame)
        s.place(s.mesh(shape, 20000), (0.0, 0.0, 0.0), 5.5 if shape == "soup" else 3.6, moving=bool(seed % 2))
        for k in range(int(rng.integers(3, 7))):
            s.sphere((0.0, 0.0, -1.0), 3.0, (0.3, 0.9))
        for k in range(int(rng.integers(1, 3))):
            s.plane(k)
        s.sphere_lights(1, None)
    elif family == "seven":
        cells, radius = _cells(rng, 7)
        for shape, c in zip(s.shapes(7), cells):
            s.place(s.mesh(shape, int(rng.integers(500, 5001))), c, radius)
        s.plane(0)
        for k in range(int(rng.integers(0, 3))):
            s.sphere((0.0, 0.0, -2.0), 3.0, (0.3, 0.8))
        if most_lights:
            s.sphere_lights(MAX_LIGHTS, MAX_LIGHT_SAMPLES)
        else:
            s.sphere_lights(int(rng.integers(1, MAX_LIGHTS + 1)), int(rng.integers(2, MAX_LIGHT_SAMPLES + 1)))
    elif family == "twelve":
        cells, radius = _cells(rng, 12)
        sizes = [9, 33, 150, 5000] + [int(v) for v in np.exp(rng.uniform(np.log(9.0), np.log(5000.0), 8)).astype(int)]
        sizes = [sizes[k] for k in rng.permutation(12)]
        for shape, n, c in zip(s.shapes(12), sizes, cells):
            s.place(s.mesh(shape if n >= 64 else str(rng.choice(["soup", "sheet"])), n), c, radius)
        s.plane(1)
        s.sphere_lights(int(rng.integers(1, 3)), None)
    elif family == "instances":
        names = [s.mesh(str(rng.choice(CLOSED)), int(rng.integers(2000, 4001))), s.mesh("soup", int(rng.integers(800, 2001)))]
        cells, radius = _cells(rng, 16)
        for k, c in enumerate(cells):
            s.place(names[int(rng.integers(0, 2)) if k >= 2 else k], c, radius, moving=(k % 3 == 0))
        s.plane(0)
        s.sphere_lights(int(rng.integers(1, 3)), None)
    elif family == "mesh_light":
        cells, radius = _cells(rng, 4)
        s.materials.append(material(rng, "glow", True))
        s.place(s.mesh(str(rng.choice(CLOSED)), int(rng.integers(2000, 6001))), cells[0], radius, mat="glow", light_samples=int(rng.integers(2, 4)))
        for shape, c in zip(s.shapes(3), cells[1:]):
            s.place(s.mesh(shape, int(rng.integers(300, 3001))), c, radius)
        s.plane(0)
        s.plane(1)
        for k in range(int(rng.integers(2, 5))):
            s.sphere((0.0, 0.0, 1.0), 3.0, (0.2, 0.5))
    elif family == "beyond_flat":
        total, nmesh, nplanes = int(rng.integers(70, 101)), int(rng.integers(3, 11)), int(rng.integers(0, 8))
        nlights = int(rng.integers(1, 3))
        cells, radius = _cells(rng, nmesh)
        kinds = ["mesh"]*nmesh + ["plane"]*nplanes + ["sphere"]*(total - nmesh - nplanes - nlights)
        kinds = [kinds[k] for k in rng.permutation(len(kinds))]           # (meshes and planes anywhere in the list)
        shapes, planes = s.shapes(nmesh), 0
        for kind in kinds:
            if kind == "mesh":
                s.place(s.mesh(shapes.pop(), int(rng.integers(500, 4001))), cells.pop(), radius)
            elif kind == "plane":
                s.plane(planes)
                planes += 1
            else:
                s.sphere((0.0, 0.0, -2.5), 3.5, (0.1, 0.35))
        s.sphere_lights(nlights, None)
    else:
        raise KeyError(family)
    return s.text()


if __name__ == "__main__":
    sys.stdout.write(scene_text(sys.argv[1], int(sys.argv[2])))

"""Headless stand-in for the caller of the boundary -- the role src/main.cpp plays behind GLUT.

    python -m tinsel_amd.headless [-spp=N] [-width=W] [-height=H] [-exposure=E] [-maxdepth=D]
                                  [-nlm=RADIUS[,FALLOFF]] [-rr=BOUNCE] [-out=image.png|image.pfm] [-save=state.npz] [-resume=state.npz]
                                  [-complexity=rays|nodes|tris|prims] [-firsthit=buffers.npz]
                                  [-irradiance=bake.npz] [-irradiance_spp=N]
                                  [-probes=probes.npz -probes_at=positions.npy] [-probes_spp=N] [-probes_order=0|1|2]
                                  [-features=features.npz] [-features_spp=N] [-denoise[=RADIUS]]
                                  [-mattes=FILE.npz] [-mattes_spp=N] [-mattes_slots=K]
                                  [-lightgroups=FILE.npz] [-lightgroups_spp=N]
                                  [-depthplanes=FILE.npz] [-depthplanes_spp=N] [-depthplanes_at=D1,D2,...]
                                  [-views=FILE.npz -views_orbit=N] [-views_spp=S] [-views_center=X,Y,Z]
                                  [-samplemap=COUNTS.npy -samplemap_out=FILE.npz] [-samplemap_begin=N]
                                  scene.pack

Conventions kept from main.cpp:
  * the LAST argument is the input file (main.cpp:97-101); here a scene pack written by the reference's own loader +
    Scene::Build (tests/golden/make_golden.py; .tin parsing is the reference's loader and stays there -- the C++ shim
    shim/tinsel_headless.cpp takes .tin directly);
  * `-key=value` overrides are applied after the scene's own options (main.cpp:143-149), `-spp` sets
    options.maxSamples;
  * a frame = 16 calls of Renderer::Render, one more sample per pixel each (main.cpp:242-250), then the display
    stage (normalise, ToneMap, LinearToSrgb, optional NonLocalMeansFilter: main.cpp:258-282) and one progress line
    "<samples> render: (ms) total: (ms)" (main.cpp:303);
  * when the sample count reaches maxSamples the image is written with WritePng's conversion (main.cpp:307-312).
  * BATCH / animation mode (main.cpp:104-118, 314-327): a `%` in the file name makes it a printf pattern over the frame index 0, 1, 2, ...;
    every frame renders maxSamples and is written to `<frame file>.png` (or `-out=pattern-with-%d`), until a frame's file does not exist.
    The reference deletes its renderer and re-runs Init per frame -- loader, Scene::Build, a new GpuRenderer: every mesh uploaded again.
    Here ONE renderer lives through the batch: where frame k + 1 is frame k with other primitive transforms (a rigid animation) the moved
    primitives' records are rewritten in place and the scene level rebuilt from the frame's own nodes (HipRenderer.update_scene:
    tinsel_hip_set_primitive_transform + tinsel_hip_rebuild_scene) -- the frames' PNGs are those of fresh renderers byte for byte
    (tests/test_gpu_display.py) -- and only a frame that differs in more is re-created.  Each frame prints what it cost to get ready.
Beyond it: `.pfm` output of the normalised linear image (PfmSave layout), and -save / -resume of the accumulator
(tinsel_hip_write_accum) so a long render can be continued bit-exactly.
-complexity=CHANNEL draws the reference's eComplexity view (RenderMode, render.h:42-47; main.cpp binds it to key 2 and no
renderer of the reference draws it): the traversal-cost map of maxSamples path-traced passes (HipRenderer.render_cost) instead of
the image.  -out gets the heat map of CHANNEL's mean per sample (display.cost_heatmap) as a PNG, or those raw means as a PFM; the
frame's mean per sample of all four channels is printed.
-firsthit=FILE.npz writes the first-hit buffers of the scene's camera at the frame size (HipRenderer.first_hit: `t` [H, W], `primitive`
[H, W], -1 where the ray leaves the scene, `normal` [H, W, 3] turned towards the camera; the pose of time 1, as the normals view) and
exits without rendering: what a denoiser or a compositor reads beside the image.
-irradiance=FILE.npz bakes the irradiance at those first-hit points (HipRenderer.first_hit_points: moved off the surface along the turned
normal by the reference's ray epsilon) with a gather query in cosine mode, -irradiance_spp paths per point (default 64) to -maxdepth:
`irradiance` [H, W, 3] = the mean radiance * pi, 0 where the ray left the scene, with `t`, `primitive` and `normal` beside it; point k
(the hit pixels in row order) draws from the seeds k*spp .. k*spp + spp - 1.  Exits without rendering, like -firsthit: the options that
belong to a render (-out, -save, -resume, -nlm, -spp), -firsthit, -complexity and batch mode are refused beside it.
-probes=FILE.npz bakes light probes at the positions of -probes_at=FILE.npy ([n, 3], scene units) with an SH gather query
(HipRenderer.gather_sh) in sphere mode, -probes_spp paths per probe (default 1024, 1 .. 65536) to -maxdepth, bands 0 .. -probes_order
(default 2): `sh` [n, C, 3] float32, C = (order + 1)^2 = 4 pi * the mean of radiance * Y_i over the probe's paths, the product taken in
float32 -- the SH coefficients of the incident radiance, which tinsel_amd.sh_irradiance turns into the irradiance for any normal -- with
`positions` beside it; probe k draws from the seeds k*spp .. k*spp + spp - 1 at time 1.  Exits without rendering: the options -irradiance
refuses are refused beside it, and so is -irradiance.
-features=FILE.npz writes, beside a normal render, the guide buffers a denoiser or a compositor takes (HipRenderer.features): the first-hit
albedo, shading normal and depth of the render's own camera samples of passes [0, -features_spp) (default min(spp, 16)), reconstructed with
the render's filter exactly as the image is.  The file holds the raw planes `albedo_plane`, `normal_plane`, `depth_plane` ([H, W, 4]
float32: weighted sum xyz, weight sum w) and tinsel_amd.feature_images of them: `albedo` [H, W, 3], `normal` [H, W, 3] (unit length),
`depth`, `depth_variance`, `coverage` [H, W], and `passes`.  Refused with batch mode, -resume (its passes are not [0, N)), -complexity,
-firsthit, -irradiance and -probes, which render no image.
-mattes=FILE.npz writes, beside a normal render, the ID mattes a compositor takes (HipRenderer.id_mattes): per pixel the ranked list of
(primitive id, filter-weight sum) pairs of the render's own camera samples of passes [0, -mattes_spp) (default min(spp, 16), as
-features_spp), -mattes_slots pairs per pixel (default 6, 1 .. 8), filtered with the render's filter exactly as the image is.  The file
holds `ids` [K, H, W] int32 (-1: the sample left the scene, -2: an unused slot), `weights` [K, H, W], `residual` [H, W], `total` [H, W]
and `passes`; tinsel_amd.matte turns them into the coverage of a set of primitives.  Refused with what -features is refused with.
-lightgroups=FILE.npz writes, beside a normal render, the light groups a compositor re-balances lights with (HipRenderer.light_groups):
the render's own passes [0, -lightgroups_spp) (default min(spp, 16), as -features_spp) split by which emitter produced the radiance, one
plane per group of tinsel_amd.default_light_groups -- every emitting primitive its own, the environment last.  The file holds `planes`
[G, H, W, 4] float32 (accumulators: the render's clamp applies per plane), `group_of_primitive`, `env_group`, `names` and `passes`;
tinsel_amd.relight mixes the planes.  Refused with what -features is refused with.
-depthplanes=FILE.npz writes, beside a normal render, the beauty at several path depths from one trace (HipRenderer.depth_planes): the
render's own passes [0, -depthplanes_spp) (default min(spp, 16), as -features_spp), one plane per depth of -depthplanes_at (strictly
ascending, 1 .. 64, 16 at most; default 1 .. the render's max depth) -- plane k what the render gives with -maxdepth=depths[k].  The file
holds `planes` [n, H, W, 4] float32 (accumulators: the render's clamp applies per plane), `depths` and `passes`;
tinsel_amd.depth_contributions turns the planes into direct light and each further bounce's share.  Refused with what -features is
refused with.
-views=FILE.npz -views_orbit=N writes, beside a normal render, a turntable of the scene in one call (HipRenderer.views): N views of the
scene's camera turned about the vertical through -views_center (default: what the camera sees at the centre of the frame, first_hit; the
origin if that ray leaves the scene) by tinsel_amd.orbit_cameras, passes [0, -views_spp) (default min(spp, 16), as -features_spp) each --
view 0 is the render's own first passes.  The file holds `planes` [N, H, W, 4] float32 (accumulators), `cameras` [N, 10] float32 (position,
rotation x y z w, fov, shutter start and end), `center` and `passes`.  Refused with what -features is refused with.
-samplemap=COUNTS.npy -samplemap_out=FILE.npz writes, beside a normal render, the plane of a sample-map call (HipRenderer.sample_map):
COUNTS.npy holds a uint16 array [H, W], the number of passes every pixel gets -- pixel (i, j) the samples a render gives it in the passes
-samplemap_begin (default 0) .. -samplemap_begin + COUNTS[j, i] - 1, and none beyond; tinsel_amd.crop_sample_map makes a crop.  The file
holds `plane` [H, W, 4] float32 (an accumulator: divide by the weight channel), `counts` and `pass_begin`.  Refused with what -features is
refused with.
-denoise[=RADIUS] does a normal render, then takes the features of its passes [0, spp), denoises the accumulator with the library's
defaults (HipRenderer.denoise: the feature-guided filter on linear radiance; RADIUS 1 .. 8 replaces the default search radius), runs the
display stage on the denoised image (HipRenderer.present_image) and writes that to -out (a .pfm gets the denoised linear radiance).
Refused with what -features is refused with.

No CPU fallback: without a GPU and the HIP library this exits with the library's error.
"""
import os
import sys
import time

import numpy as np

from . import abi
from .display import COST_CHANNELS, cost_heatmap, cost_mean, write_pfm, write_png
from .renderer import Scene, camera_rays, create_gpu_renderer, default_light_groups, denoise_params, feature_images, gather_points, orbit_cameras

FRAME_PASSES = 16          # numSamples of main.cpp:240


def parse_args(argv):
    if len(argv) < 2:
        raise SystemExit(__doc__)
    cfg = {"file": argv[-1], "out": None, "nlm": 0, "nlm_falloff": 200.0, "save": None, "resume": None, "complexity": None, "firsthit": None, "irradiance": None,
           "irradiance_spp": 64, "probes": None, "probes_at": None, "probes_spp": 1024, "probes_order": 2, "features": None, "features_spp": None,
           "mattes": None, "mattes_spp": None, "mattes_slots": None, "lightgroups": None, "lightgroups_spp": None,
           "depthplanes": None, "depthplanes_spp": None, "depthplanes_at": None,
           "views": None, "views_orbit": None, "views_spp": None, "views_center": None,
           "samplemap": None, "samplemap_out": None, "samplemap_begin": None,
           "denoise": None, "over": {}}
    for a in argv[1:-1]:
        if a == "-denoise":
            cfg["denoise"] = 0          # the default radius
            continue
        if not a.startswith("-") or "=" not in a:
            raise SystemExit("unrecognised argument %r\n%s" % (a, __doc__))
        k, v = a[1:].split("=", 1)
        if k in ("spp", "width", "height", "maxdepth", "rr"):
            cfg["over"][k] = int(v)
        elif k == "exposure":
            cfg["over"][k] = float(v)
        elif k == "nlm":
            parts = v.split(",")
            cfg["nlm"] = int(parts[0])
            if len(parts) > 1:
                cfg["nlm_falloff"] = float(parts[1])
        elif k in ("out", "save", "resume", "firsthit", "irradiance", "probes", "probes_at", "features", "mattes", "lightgroups", "depthplanes", "views", "samplemap",
                   "samplemap_out"):
            cfg[k] = v
        elif k == "denoise":
            cfg[k] = int(v)
            if not 1 <= cfg[k] <= 8:
                raise SystemExit("-denoise=%s: want a radius 1 .. 8" % v)
        elif k == "features_spp":
            cfg[k] = int(v)
            if cfg[k] < 1:
                raise SystemExit("-features_spp=%s: want 1 or more" % v)
        elif k in ("views_orbit", "views_spp"):
            cfg[k] = int(v)
            if not 1 <= cfg[k] <= (abi.MAX_VIEWS if k == "views_orbit" else 1 << 20):
                raise SystemExit("-%s=%s: want 1 or more%s" % (k, v, " and %d at most" % abi.MAX_VIEWS if k == "views_orbit" else ""))
        elif k == "samplemap_begin":
            cfg[k] = int(v)
            if not 0 <= cfg[k] < 1 << 32:
                raise SystemExit("-samplemap_begin=%s: want a pass index, 0 or more" % v)
        elif k == "views_center":
            cfg[k] = tuple(float(x) for x in v.split(","))
            if len(cfg[k]) != 3:
                raise SystemExit("-views_center=%s: want X,Y,Z" % v)
        elif k == "lightgroups_spp":
            cfg[k] = int(v)
            if cfg[k] < 1:
                raise SystemExit("-lightgroups_spp=%s: want 1 or more" % v)
        elif k == "depthplanes_spp":
            cfg[k] = int(v)
            if cfg[k] < 1:
                raise SystemExit("-depthplanes_spp=%s: want 1 or more" % v)
        elif k == "depthplanes_at":
            try:
                cfg[k] = tuple(int(x) for x in v.split(","))
            except ValueError:
                raise SystemExit("-depthplanes_at=%s: want D1,D2,..." % v)
            if not 1 <= len(cfg[k]) <= abi.MAX_DEPTH_PLANES or cfg[k][0] < 1 or cfg[k][-1] > abi.MAX_PLANE_DEPTH or \
                    any(b <= a for a, b in zip(cfg[k], cfg[k][1:])):
                raise SystemExit("-depthplanes_at=%s: want 1 .. %d depths, strictly ascending, in 1 .. %d" % (v, abi.MAX_DEPTH_PLANES, abi.MAX_PLANE_DEPTH))
        elif k == "mattes_spp":
            cfg[k] = int(v)
            if cfg[k] < 1:
                raise SystemExit("-mattes_spp=%s: want 1 or more" % v)
        elif k == "mattes_slots":
            cfg[k] = int(v)
            if not 1 <= cfg[k] <= abi.ID_MAX_SLOTS:
                raise SystemExit("-mattes_slots=%s: want 1 .. %d" % (v, abi.ID_MAX_SLOTS))
        elif k == "probes_spp":
            cfg[k] = int(v)
            if not 1 <= cfg[k] <= 65536:
                raise SystemExit("-probes_spp=%s: want 1 .. 65536" % v)
        elif k == "probes_order":
            if v not in ("0", "1", "2"):
                raise SystemExit("-probes_order=%s: want 0, 1 or 2" % v)
            cfg[k] = int(v)
        elif k == "irradiance_spp":
            cfg[k] = int(v)
            if not 1 <= cfg[k] <= 65536:
                raise SystemExit("-irradiance_spp=%s: want 1 .. 65536" % v)
        elif k == "complexity":
            if v not in COST_CHANNELS:
                raise SystemExit("-complexity=%s: want one of %s" % (v, "|".join(COST_CHANNELS)))
            cfg[k] = v
        else:
            raise SystemExit("unrecognised option -%s\n%s" % (k, __doc__))
    return cfg


def apply_overrides(scene, over):
    cam, opt = scene.camera, scene.options
    if "spp" in over:
        opt.max_samples = over["spp"]
    elif opt.max_samples >= 2**31 - 1:
        # the interactive reference renders until closed (maxSamples = INT_MAX, main.cpp:189); a batch run needs an end
        opt.max_samples = 64
        print("no -spp given and the scene sets no sample limit: rendering 64 spp")
    opt.width = over.get("width", opt.width)
    opt.height = over.get("height", opt.height)
    opt.max_depth = over.get("maxdepth", opt.max_depth)
    opt.exposure = over.get("exposure", opt.exposure)
    return cam, opt


def render_frame(r, cam, opt, cfg, samples=0):
    """the progressive loop of main.cpp:242-303 up to maxSamples; returns (presented image, samples)"""
    image = None
    while samples < opt.max_samples:
        ts = time.perf_counter()
        n = min(FRAME_PASSES, opt.max_samples - samples)
        r.render(cam, opt, passes=n, readback=False)
        tr = time.perf_counter()
        image = r.present(opt, cfg["nlm"], cfg["nlm_falloff"])
        samples += n
        te = time.perf_counter()
        print("%d render: (%.4fms) total: (%.4fms)" % (samples, (tr - ts)*1000.0, (te - ts)*1000.0), flush=True)
    if image is None:
        image = r.present(opt, cfg["nlm"], cfg["nlm_falloff"])
    return image, samples


def batch(cfg):
    """main.cpp's batch mode (:104-118, :314-327) with ONE renderer for the whole animation where the frames allow it."""
    over = cfg["over"]
    r, prev, index, ready_ms = None, None, 0, []
    while True:
        name = cfg["file"] % index
        if not os.path.exists(name):
            if index == 0:
                raise SystemExit("Couldn't open %s for reading." % name)       # (main.cpp:131-135)
            break
        t0 = time.perf_counter()
        scene = Scene.load_pack(name)
        cam, opt = apply_overrides(scene, over)
        how = "created"
        if r is not None and r.update_scene(prev, scene):
            how = "updated in place"
        else:
            if r is not None:
                r.close()
                how = "re-created (the frame differs in more than transforms)"
            r = create_gpu_renderer(scene)
            if over.get("rr", 0) > 0:
                r.set_russian_roulette(over["rr"])
        r.init(opt.width, opt.height)
        r.set_pass_index(0)             # every frame starts its seeds where a fresh renderer would
        ms = (time.perf_counter() - t0)*1000.0
        ready_ms.append((how, ms))
        print("frame %d: %s: renderer %s in %.3fms" % (index, name, how, ms), flush=True)
        image, _ = render_frame(r, cam, opt, cfg)
        out = (cfg["out"] % index) if (cfg["out"] and "%" in cfg["out"]) else name + ".png"      # (main.cpp:113-115: input + ".png")
        write_png(out, image)
        print("wrote %s" % out, flush=True)
        prev = scene
        index += 1
    if r is not None:
        r.close()
    inplace = [ms for how, ms in ready_ms[1:] if how == "updated in place"]
    print("%d frames; first renderer ready in %.3fms%s" % (index, ready_ms[0][1],
          "; %d later frames updated in place in %.3fms on average (the reference re-creates: the first frame's cost every time)" % (
              len(inplace), sum(inplace)/len(inplace)) if inplace else ""))
    return 0


def complexity(r, cam, opt, cfg):
    """-complexity: the cost map of passes [0, maxSamples) instead of the image (tinsel_hip_render_cost)"""
    ts = time.perf_counter()
    counts = r.render_cost(cam, opt, 0, opt.max_samples)
    print("%d complexity: (%.4fms)" % (opt.max_samples, (time.perf_counter() - ts)*1000.0), flush=True)
    paths = float(opt.width)*opt.height*opt.max_samples
    print("mean per sample: " + " ".join("%s=%.4f" % (name, counts[..., c].sum(dtype=np.float64)/paths)
                                         for c, name in enumerate(COST_CHANNELS)))
    if cfg["out"]:
        if cfg["out"].endswith(".pfm"):
            write_pfm(cfg["out"], np.repeat(cost_mean(counts, cfg["complexity"], opt.max_samples)[..., None], 3, axis=2).astype(np.float32))
        else:
            write_png(cfg["out"], cost_heatmap(counts, cfg["complexity"], samples=opt.max_samples))
        print("wrote %s" % cfg["out"])


def irradiance(r, cam, opt, cfg):
    """-irradiance: a gather query in cosine mode at the frame's first-hit points"""
    spp = cfg["irradiance_spp"]
    points, t, primitive, normal = r.first_hit_points(cam, opt.width, opt.height)
    hit = primitive >= 0
    ts = time.perf_counter()
    mean = r.gather(gather_points(points[hit], normal[hit], spp), spp, opt.max_depth, "cosine")
    ms = (time.perf_counter() - ts)*1000.0
    out = np.zeros((opt.height, opt.width, 3), np.float32)
    out[hit] = mean[:, :3]*np.float32(np.pi)
    np.savez(cfg["irradiance"], irradiance=out, t=t, primitive=primitive, normal=normal)
    print("wrote %s: %dx%d, %d points x %d paths in %.3fms" % (cfg["irradiance"], opt.width, opt.height, int(hit.sum()), spp, ms))


def probes(r, opt, cfg):
    """-probes: an SH gather query in sphere mode at the given positions"""
    spp, order = cfg["probes_spp"], cfg["probes_order"]
    pos = np.load(cfg["probes_at"])
    if pos.ndim != 2 or pos.shape[1] != 3:
        raise SystemExit("-probes_at=%s: want an [n, 3] array of positions, got %s" % (cfg["probes_at"], pos.shape))
    pos = np.ascontiguousarray(pos, np.float32)
    ts = time.perf_counter()
    mean = r.gather_sh(gather_points(pos, np.zeros_like(pos), spp), spp, opt.max_depth, order, "sphere")
    ms = (time.perf_counter() - ts)*1000.0
    np.savez(cfg["probes"], sh=mean[:, :, :3]*np.float32(4.0*np.pi), positions=pos)
    print("wrote %s: %d probes x %d paths, bands 0..%d in %.3fms" % (cfg["probes"], len(pos), spp, order, ms))


def features(r, cam, opt, cfg):
    """-features: the guide buffers of the render's own samples of passes [0, N) (tinsel_hip_render_features)"""
    n = cfg["features_spp"] if cfg["features_spp"] else max(1, min(int(opt.max_samples), FRAME_PASSES))
    ts = time.perf_counter()
    planes = r.features(cam, opt, 0, n)
    ms = (time.perf_counter() - ts)*1000.0
    images = feature_images(planes)
    np.savez(cfg["features"], passes=np.int64(n), **{k + "_plane": v for k, v in planes.items()}, **images)
    print("wrote %s: %dx%d, %d passes in %.3fms, coverage %.4f" % (cfg["features"], opt.width, opt.height, n, ms, float(images["coverage"].mean())))


def mattes(r, cam, opt, cfg):
    """-mattes: the ranked id lists of the render's own samples of passes [0, N) (tinsel_hip_render_id_mattes)"""
    n = cfg["mattes_spp"] if cfg["mattes_spp"] else max(1, min(int(opt.max_samples), FRAME_PASSES))
    slots = cfg["mattes_slots"] if cfg["mattes_slots"] else 6
    ts = time.perf_counter()
    m = r.id_mattes(cam, opt, 0, n, slots)
    ms = (time.perf_counter() - ts)*1000.0
    np.savez(cfg["mattes"], passes=np.int64(n), **m)
    print("wrote %s: %dx%d, %d passes, %d slots in %.3fms, %d pixels with a residual" % (cfg["mattes"], opt.width, opt.height, n, slots, ms,
                                                                                       int((m["residual"] > 0).sum())))


def lightgroups(r, scene, cam, opt, cfg):
    """-lightgroups: the render's own samples of passes [0, N) split per emitter group (tinsel_hip_render_light_groups)"""
    n = cfg["lightgroups_spp"] if cfg["lightgroups_spp"] else max(1, min(int(opt.max_samples), FRAME_PASSES))
    table, env, names = default_light_groups(scene)
    if not names:
        raise SystemExit("-lightgroups: the scene has no emitter and no environment")
    ts = time.perf_counter()
    planes = r.light_groups(cam, opt, 0, n, table, env)
    ms = (time.perf_counter() - ts)*1000.0
    np.savez(cfg["lightgroups"], passes=np.int64(n), planes=planes, group_of_primitive=table, env_group=np.int64(env), names=np.array(names))
    print("wrote %s: %dx%d, %d passes, %d groups (%s) in %.3fms" % (cfg["lightgroups"], opt.width, opt.height, n, len(names), ", ".join(names), ms))


def depthplanes(r, cam, opt, cfg):
    """-depthplanes: the render's own samples of passes [0, N) at several path depths (tinsel_hip_render_depth_planes)"""
    n = cfg["depthplanes_spp"] if cfg["depthplanes_spp"] else max(1, min(int(opt.max_samples), FRAME_PASSES))
    depths = cfg["depthplanes_at"]
    if depths is None:
        if not 1 <= int(opt.max_depth) <= abi.MAX_DEPTH_PLANES:
            raise SystemExit("-depthplanes: the render's max depth is %d, name %d depths at most with -depthplanes_at" % (int(opt.max_depth), abi.MAX_DEPTH_PLANES))
        depths = tuple(range(1, int(opt.max_depth) + 1))
    ts = time.perf_counter()
    planes = r.depth_planes(cam, opt, 0, n, depths)
    ms = (time.perf_counter() - ts)*1000.0
    np.savez(cfg["depthplanes"], passes=np.int64(n), planes=planes, depths=np.array(depths, np.int32))
    print("wrote %s: %dx%d, %d passes, %d depths (%s) in %.3fms" % (cfg["depthplanes"], opt.width, opt.height, n, len(depths),
                                                                  ", ".join(str(d) for d in depths), ms))


def views(r, cam, opt, cfg):
    """-views: a turntable of N cameras about the vertical through the centre, the passes [0, S) of each in one call (tinsel_hip_render_views)"""
    n = cfg["views_spp"] if cfg["views_spp"] else max(1, min(int(opt.max_samples), FRAME_PASSES))
    center = cfg["views_center"]
    if center is None:
        t, primitive, _ = r.first_hit(cam, opt.width, opt.height)
        j, i = opt.height//2, opt.width//2
        center = (0.0, 0.0, 0.0)
        if primitive[j, i] >= 0:
            origin, directions = camera_rays(cam, opt.width, opt.height)
            center = tuple(float(v) for v in origin + float(t[j, i])*directions[j, i])
    cams = orbit_cameras(cam, center, cfg["views_orbit"])
    ts = time.perf_counter()
    planes = r.views(cams, opt, 0, n)
    ms = (time.perf_counter() - ts)*1000.0
    table = np.array([tuple(c.position) + tuple(c.rotation) + (c.fov, c.shutter_start, c.shutter_end) for c in cams], np.float32)
    np.savez(cfg["views"], passes=np.int64(n), planes=planes, cameras=table, center=np.array(center, np.float32))
    print("wrote %s: %d views of %dx%d, %d passes each, about (%g, %g, %g) in %.3fms" % ((cfg["views"], len(cams), opt.width, opt.height, n) + tuple(center) + (ms,)))


def samplemap(r, cam, opt, cfg):
    """-samplemap: the plane of one sample-map call (tinsel_hip_render_sample_map) with the counts of a .npy file"""
    counts = np.load(cfg["samplemap"])
    if counts.dtype != np.uint16 or counts.shape != (opt.height, opt.width):
        raise SystemExit("-samplemap=%s: want a uint16 array [%d, %d], got %s %s" % (cfg["samplemap"], opt.height, opt.width, counts.dtype, counts.shape))
    begin = cfg["samplemap_begin"] or 0
    ts = time.perf_counter()
    plane = r.sample_map(cam, opt, counts, pass_begin=begin)
    ms = (time.perf_counter() - ts)*1000.0
    np.savez(cfg["samplemap_out"], plane=plane, counts=counts, pass_begin=np.int64(begin))
    print("wrote %s: %dx%d, %d samples on %d pixels (up to %d a pixel) from pass %d in %.3fms" % (
        cfg["samplemap_out"], opt.width, opt.height, int(counts.sum(dtype=np.int64)), int((counts > 0).sum()), int(counts.max()), begin, ms))


def denoise(r, cam, opt, cfg, samples):
    """-denoise: the features of the render's own passes, the denoise stage on the accumulator, the display stage on its result;
    returns (presented image, denoised linear image)"""
    ts = time.perf_counter()
    params = denoise_params(radius=cfg["denoise"]) if cfg["denoise"] else denoise_params()
    linear = r.denoise(r.features(cam, opt, 0, samples), params)
    image = r.present_image(linear, opt, cfg["nlm"], cfg["nlm_falloff"])
    print("denoise: radius %d, features of %d passes (%.4fms)" % (params.radius, samples, (time.perf_counter() - ts)*1000.0), flush=True)
    return image, linear


def main(argv=None):
    cfg = parse_args(sys.argv if argv is None else argv)
    if cfg["features_spp"] and not cfg["features"]:
        raise SystemExit("-features_spp goes with -features=OUT.npz")
    if cfg["features"] and ("%" in cfg["file"] or cfg["resume"] or cfg["complexity"] or cfg["firsthit"] or cfg["irradiance"] or cfg["probes"] or
                            cfg["probes_at"]):
        raise SystemExit("-features writes the guide buffers of a normal render's passes [0, N): no batch mode, no -resume, -complexity, "
                         "-firsthit, -irradiance or -probes")
    if (cfg["mattes_spp"] or cfg["mattes_slots"]) and not cfg["mattes"]:
        raise SystemExit("-mattes_spp and -mattes_slots go with -mattes=OUT.npz")
    if cfg["mattes"] and ("%" in cfg["file"] or cfg["resume"] or cfg["complexity"] or cfg["firsthit"] or cfg["irradiance"] or cfg["probes"] or
                          cfg["probes_at"]):
        raise SystemExit("-mattes writes the ID mattes of a normal render's passes [0, N): no batch mode, no -resume, -complexity, "
                         "-firsthit, -irradiance or -probes")
    if cfg["lightgroups_spp"] and not cfg["lightgroups"]:
        raise SystemExit("-lightgroups_spp goes with -lightgroups=OUT.npz")
    if cfg["lightgroups"] and ("%" in cfg["file"] or cfg["resume"] or cfg["complexity"] or cfg["firsthit"] or cfg["irradiance"] or cfg["probes"] or
                               cfg["probes_at"]):
        raise SystemExit("-lightgroups writes the light groups of a normal render's passes [0, N): no batch mode, no -resume, -complexity, "
                         "-firsthit, -irradiance or -probes")
    if (cfg["depthplanes_spp"] or cfg["depthplanes_at"]) and not cfg["depthplanes"]:
        raise SystemExit("-depthplanes_spp and -depthplanes_at go with -depthplanes=OUT.npz")
    if cfg["depthplanes"] and ("%" in cfg["file"] or cfg["resume"] or cfg["complexity"] or cfg["firsthit"] or cfg["irradiance"] or cfg["probes"] or
                               cfg["probes_at"]):
        raise SystemExit("-depthplanes writes the depth planes of a normal render's passes [0, N): no batch mode, no -resume, -complexity, "
                         "-firsthit, -irradiance or -probes")
    if bool(cfg["views"]) != bool(cfg["views_orbit"]) or ((cfg["views_spp"] or cfg["views_center"]) and not cfg["views"]):
        raise SystemExit("-views=OUT.npz and -views_orbit=N go together; -views_spp and -views_center go with them")
    if cfg["views"] and ("%" in cfg["file"] or cfg["resume"] or cfg["complexity"] or cfg["firsthit"] or cfg["irradiance"] or cfg["probes"] or
                         cfg["probes_at"]):
        raise SystemExit("-views writes a turntable beside a normal render: no batch mode, no -resume, -complexity, -firsthit, -irradiance "
                         "or -probes")
    if bool(cfg["samplemap"]) != bool(cfg["samplemap_out"]) or (cfg["samplemap_begin"] is not None and not cfg["samplemap"]):
        raise SystemExit("-samplemap=COUNTS.npy and -samplemap_out=OUT.npz go together; -samplemap_begin goes with them")
    if cfg["samplemap"] and ("%" in cfg["file"] or cfg["resume"] or cfg["complexity"] or cfg["firsthit"] or cfg["irradiance"] or cfg["probes"] or
                             cfg["probes_at"]):
        raise SystemExit("-samplemap writes a sample-map plane beside a normal render: no batch mode, no -resume, -complexity, -firsthit, "
                         "-irradiance or -probes")
    if cfg["denoise"] is not None and ("%" in cfg["file"] or cfg["resume"] or cfg["complexity"] or cfg["firsthit"] or cfg["irradiance"] or cfg["probes"] or
                                       cfg["probes_at"]):
        raise SystemExit("-denoise filters a normal render with the guide buffers of its passes [0, N): no batch mode, no -resume, -complexity, "
                         "-firsthit, -irradiance or -probes")
    if cfg["complexity"] and ("%" in cfg["file"] or cfg["save"] or cfg["resume"]):
        raise SystemExit("-complexity renders one cost map: no batch mode, -save or -resume")
    if cfg["firsthit"] and ("%" in cfg["file"] or cfg["complexity"]):
        raise SystemExit("-firsthit writes one frame's buffers: no batch mode, no -complexity")
    if cfg["irradiance"] and ("%" in cfg["file"] or cfg["complexity"] or cfg["firsthit"] or cfg["out"] or cfg["save"] or cfg["resume"] or
                              cfg["nlm"] or "spp" in cfg["over"]):
        raise SystemExit("-irradiance bakes one frame's points and renders nothing: no batch mode, no -complexity, -firsthit, -out, -save, "
                         "-resume, -nlm or -spp (the paths per point are -irradiance_spp)")
    if bool(cfg["probes"]) != bool(cfg["probes_at"]):
        raise SystemExit("-probes=OUT.npz and -probes_at=IN.npy go together")
    if cfg["probes"] and ("%" in cfg["file"] or cfg["complexity"] or cfg["firsthit"] or cfg["irradiance"] or cfg["out"] or cfg["save"] or cfg["resume"] or
                          cfg["nlm"] or "spp" in cfg["over"]):
        raise SystemExit("-probes bakes light probes and renders nothing: no batch mode, no -complexity, -firsthit, -irradiance, -out, -save, "
                         "-resume, -nlm or -spp (the paths per probe are -probes_spp)")
    if "%" in cfg["file"]:
        return batch(cfg)
    t0 = time.perf_counter()
    scene = Scene.load_pack(cfg["file"])
    cam, opt = apply_overrides(scene, cfg["over"])
    over = cfg["over"]

    r = create_gpu_renderer(scene)
    if cfg["firsthit"]:
        t, primitive, normal = r.first_hit(cam, opt.width, opt.height)
        r.close()
        np.savez(cfg["firsthit"], t=t, primitive=primitive, normal=normal)
        print("wrote %s: %dx%d, %d pixels hit" % (cfg["firsthit"], opt.width, opt.height, int((primitive >= 0).sum())))
        return 0
    if over.get("rr", 0) > 0:
        r.set_russian_roulette(over["rr"])       # opt-in; not the reference's behaviour (tinsel_hip.h)
    if cfg["irradiance"]:
        irradiance(r, cam, opt, cfg)
        r.close()
        return 0
    if cfg["probes"]:
        try:
            probes(r, opt, cfg)
        finally:
            r.close()
        return 0
    r.init(opt.width, opt.height)
    print("Created renderer in %fms" % ((time.perf_counter() - t0)*1000.0))
    if cfg["complexity"]:
        complexity(r, cam, opt, cfg)
        r.close()
        return 0

    samples = 0
    if cfg["resume"]:
        st = np.load(cfg["resume"])
        samples = int(st["samples"])
        r.write_accum(st["accum"], samples)

    image, samples = render_frame(r, cam, opt, cfg, samples)

    if cfg["features"]:
        features(r, cam, opt, cfg)
    if cfg["mattes"]:
        mattes(r, cam, opt, cfg)
    if cfg["lightgroups"]:
        lightgroups(r, scene, cam, opt, cfg)
    if cfg["depthplanes"]:
        depthplanes(r, cam, opt, cfg)
    if cfg["views"]:
        views(r, cam, opt, cfg)
    if cfg["samplemap"]:
        samplemap(r, cam, opt, cfg)
    linear = None
    if cfg["denoise"] is not None:
        image, linear = denoise(r, cam, opt, cfg, samples)
    if cfg["save"]:
        np.savez(cfg["save"], accum=r.read_accum(), samples=np.int64(samples))
    if cfg["out"]:
        if cfg["out"].endswith(".pfm"):
            a = r.read_accum() if linear is None else linear
            with np.errstate(all="ignore"):
                write_pfm(cfg["out"], a[..., :3]/a[..., 3:4])
        else:
            write_png(cfg["out"], image)
        print("wrote %s" % cfg["out"])
    st = r.stats()
    print("%d samples, %d rays" % (st["samples"], st["rays"]))
    r.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())

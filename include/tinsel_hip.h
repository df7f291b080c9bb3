/*
 * tinsel_hip.h -- C-ABI of the MI355X (gfx950) path-tracing back-end for Tinsel.
 *
 * This is the drop-in boundary. It replaces what the reference does behind
 *     Renderer* CreateGpuRenderer(const Scene* s);            (reference src/render.h:79)
 *     struct Renderer { Init(w,h); Render(cam, opts, out); }  (reference src/render.h:66-73)
 * which the reference implements with CUDA in src/render.cu:978-1110.
 *
 * Everything that crosses this ABI is plain pointers + sizes.  The POD records
 * below are *layout mirrors* of the reference structs (sizes/offsets asserted at
 * the bottom of this file), so a Tinsel maintainer passes `&scene->primitives[0]`,
 * `scene->bvh.nodes`, `&camera`, `&options` unchanged -- see INTEGRATION.md for
 * the ~40-line `HipRenderer : Renderer` shim (shim/hip_renderer.cpp).
 *
 * No torch types, no C++ types, no exceptions cross this boundary.  All entry
 * points return 0 on success / non-zero on failure (or NULL for constructors) and
 * leave a message retrievable with tinsel_hip_last_error().
 */
#ifndef TINSEL_HIP_H
#define TINSEL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------- */
/* POD mirrors of the reference structs                                       */

typedef struct tinsel_vec3 { float x, y, z; } tinsel_vec3;          /* maths.h:214-234  (12 B) */
typedef struct tinsel_vec4 { float x, y, z, w; } tinsel_vec4;       /* maths.h:290-312  (16 B), Color/Quat alike */

typedef struct tinsel_transform {                                   /* maths.h:575-589  (32 B) */
    tinsel_vec3 p;
    tinsel_vec4 r;      /* quaternion x,y,z,w */
    float s;
} tinsel_transform;

typedef struct tinsel_bvh_node {                                    /* bvh.h:9-20       (32 B) */
    tinsel_vec3 lower;
    tinsel_vec3 upper;
    uint32_t left_index;            /* leaf: item index */
    uint32_t right_index_leaf;      /* bits 0..30 = rightIndex, bit 31 = leaf */
} tinsel_bvh_node;

typedef struct tinsel_camera {                                      /* scene.h:11-30    (40 B) */
    tinsel_vec3 position;
    tinsel_vec4 rotation;
    float fov;
    float shutter_start;
    float shutter_end;
} tinsel_camera;

typedef struct tinsel_texture {                                     /* scene.h:33-42    (24 B) */
    float* data;
    int32_t width, height, depth;
    int32_t _pad;
} tinsel_texture;

typedef struct tinsel_material {                                    /* scene.h:45-100   (128 B) */
    tinsel_vec3 emission;
    tinsel_vec3 color;
    tinsel_vec3 absorption;
    float eta;
    float metallic;
    float subsurface;
    float specular;
    float roughness;
    float specular_tint;
    float anisotropic;
    float sheen;
    float sheen_tint;
    float clearcoat;
    float clearcoat_gloss;
    float transmission;
    int32_t _pad0;
    tinsel_texture bump_map;
    float bump;
    tinsel_vec3 bump_tile;
} tinsel_material;

enum { TINSEL_GEOM_SPHERE = 0, TINSEL_GEOM_PLANE = 1, TINSEL_GEOM_MESH = 2 };   /* scene.h:102-107 */

typedef struct tinsel_mesh_geometry {                               /* scene.h:119-135  (64 B) */
    const tinsel_vec3* positions;
    const tinsel_vec3* normals;
    const int32_t* indices;
    const tinsel_bvh_node* nodes;
    const float* cdf;
    int32_t num_vertices;
    int32_t num_indices;
    int32_t num_nodes;
    float area;
    uint64_t id;
} tinsel_mesh_geometry;

typedef struct tinsel_primitive {                                   /* scene.h:138-159  (272 B) */
    tinsel_transform start_transform;
    tinsel_transform end_transform;
    int32_t type;
    int32_t _pad0;
    union {
        struct { float radius; } sphere;
        struct { float plane[4]; } plane;
        tinsel_mesh_geometry mesh;
    } geo;
    tinsel_material material;
    int32_t light_samples;
    int32_t _pad1;
} tinsel_primitive;

enum { TINSEL_FILTER_BOX = 0, TINSEL_FILTER_GAUSSIAN = 1 };          /* render.h:7-11 */

typedef struct tinsel_filter {                                      /* render.h:13-39   (16 B) */
    int32_t type;
    float width;
    float falloff;
    float offset;       /* taken verbatim from the caller, never recomputed (loader quirk, loader.cpp:74) */
} tinsel_filter;

enum { TINSEL_MODE_NORMALS = 0, TINSEL_MODE_COMPLEXITY = 1, TINSEL_MODE_PATHTRACE = 2 }; /* render.h:42-47 */

typedef struct tinsel_options {                                     /* render.h:50-63   (48 B) */
    int32_t mode;
    int32_t width;
    int32_t height;
    tinsel_filter filter;
    float exposure;
    float limit;
    float clamp;
    int32_t max_depth;
    int32_t max_samples;
} tinsel_options;

/* Flat view of a reference `Scene` (scene.h:183-215).  `Scene` itself holds
 * std::vectors, so the C++ side of the shim walks it and fills this struct;
 * nothing behind this ABI touches libstdc++ containers. */
typedef struct tinsel_scene_desc {
    const tinsel_primitive* primitives;     /* &scene->primitives[0]; mesh pointers are HOST pointers */
    int32_t num_primitives;
    int32_t num_bvh_nodes;                  /* scene->bvh.numNodes */
    const tinsel_bvh_node* bvh_nodes;       /* scene->bvh.nodes (built by Scene::Build, scene.cpp:4-16) */
    tinsel_vec3 sky_horizon;                /* scene->sky.horizon  (scene.h:163) */
    tinsel_vec3 sky_zenith;                 /* scene->sky.zenith */
    int32_t probe_valid;                    /* scene->sky.probe.valid (probe.h:81) */
    int32_t probe_width;
    int32_t probe_height;
    int32_t _pad;
    const tinsel_vec4* probe_data;          /* probe.data,  width*height RGBA32F */
    const float* probe_pdf_x;               /* probe.pdfValuesX  [w*h] */
    const float* probe_cdf_x;               /* probe.cdfValuesX  [w*h] */
    const float* probe_pdf_y;               /* probe.pdfValuesY  [h]   */
    const float* probe_cdf_y;               /* probe.cdfValuesY  [h]   */
} tinsel_scene_desc;

/* ------------------------------------------------------------------------- */
/* The renderer object                                                        */

typedef struct tinsel_hip tinsel_hip;       /* opaque */

/* Pipeline selection (tinsel_hip_set_pipeline).  WAVEFRONT is the product path: one streaming
 * kernel per bounce over HBM ray queues with wave64 compaction.  MEGAKERNEL (one lane per whole
 * path) and WAVEFRONT_SPLIT (extend / shade / shadow kernels per bounce) are A/B arms with
 * identical per-path arithmetic. */
enum { TINSEL_PIPELINE_WAVEFRONT = 0, TINSEL_PIPELINE_MEGAKERNEL = 1, TINSEL_PIPELINE_WAVEFRONT_SPLIT = 2,
       /* PAIRED: the split pipeline re-cut for scenes with meshes in HBM -- a bounce's shadow rays and the next bounce's extension rays are
        * walked in ONE k_walk launch, ONE streaming kernel per bounce does the rest (tn_paired.h); same arithmetic, same bits */
       TINSEL_PIPELINE_WAVEFRONT_PAIRED = 4,
       /* default: WAVEFRONT (fused bounce kernel) when the whole scene is LDS-resident; else WAVEFRONT_PAIRED where every mesh is walked by
        * k_walk, nothing moves and no light is a large mesh (measured: DESIGN.md section 5), else WAVEFRONT_SPLIT */
       TINSEL_PIPELINE_AUTO = 3 };

/* Replaces GpuRenderer::GpuRenderer (render.cu:989-1053): deep-copies the scene
 * to device `device_index` (dedupes meshes by MeshGeometry::id, re-lays BVHs out
 * for 64-B two-child records, pre-gathers triangles).  The desc and everything it
 * points to may be freed once this returns. */
tinsel_hip* tinsel_hip_create(const tinsel_scene_desc* scene, int device_index);

/* Tuning: every choice between two code paths of the library that a scene or a batch size normally decides, as ONE plain
 * struct (no reference counterpart: the reference has one kernel and no choices).  Nothing here changes a result -- every
 * setting renders the same image bit for bit (tests/test_gpu_switches.py drives all of them) -- and nothing is read from the
 * caller's ENVIRONMENT: a production caller gets the defaults (tinsel_hip_create), a test or an A/B run fills the struct.
 * Convention: -1 (or 0 where stated) = "the library decides"; struct_bytes = sizeof(tinsel_hip_tuning) as the CALLER compiled
 * it (a library built against a longer struct takes the defaults for the fields the caller does not have). */
typedef struct tinsel_hip_tuning {
    uint32_t struct_bytes;
    /* ---- where the scene's data lives and how its scene level is scanned: read by tinsel_hip_create_tuned only ---- */
    int32_t flat_scan;          /* -1 auto | 0: scene level by BVH walk even where the flat scan could take it (<= 64 primitives) */
    int32_t lds_scene;          /* -1 auto | 0: the scene arena stays in HBM (never staged into LDS) */
    int32_t walk;               /* -1 auto | 0: meshes in HBM are walked inline by k_extend / k_shadow, no k_walk */
    int32_t inline_max_tris;    /* -1 default | triangles up to which a mesh rides in the arena beside a mesh in HBM */
    int32_t walk_min_tris;      /* -1 default | triangle count from which k_walk takes a mesh in HBM */
    int64_t small_mesh_bytes;   /* -1 default | size up to which a mesh rides in the arena (0: every mesh lives in HBM) */
    int64_t arena_lds_limit;    /* -1 default | arena size up to which it is staged into LDS */
    /* ---- per render: tinsel_hip_set_tuning changes them at any time between two renders ---- */
    int64_t batch_paths;        /* 0 default | path slots resident per batch (>= 65536; tinsel_hip_set_batch_paths sets the same field) */
    int32_t grid_mult;          /* 0 default (32) | upper bound of the streaming grid in workgroups per CU */
    int32_t bounce_share;       /* -1 auto | 0 / 1: k_bounce deals its workgroup's four regions to its waves as one stream: never / always */
    int32_t repack;             /* -1 auto | 0 / 1: k_bounce's per-wave shading pools: never / always (where the LDS allows) */
    int32_t tail_split;         /* -1 auto | 0 off | 1: the last tail_share of a batch in regions 1/tail_divide as long */
    float tail_share;
    int32_t tail_divide;
    int32_t shade_sorted;       /* -1 auto | 0 / 1: k_shade / k_shade_sorted */
    int32_t overlap;            /* -1 auto | 0 / 1: a batch's passes as two overlapped chunks on two streams: never / wherever it has two passes */
    int32_t scene_walk;         /* -1 auto | 0: scenes beyond the flat scan through k_extend / k_shadow instead of k_swalk */
    int32_t swalk_lds;          /* -1 auto | 0: k_swalk's 256-thread generic-pointer variant */
    int32_t accumulate;         /* 0 auto | TINSEL_ACCUMULATE_TILED / _WIDE / _PIPED (filter widths up to 1) | _FULL_WINDOW: auto, but never the support form */
    int32_t walk_block;         /* 0 auto | 256 / 1024: k_walk's workgroup size */
    int32_t walk_single;        /* -1 auto | 0: per-lane tree pointers (k_walk_rays) also for ONE walked primitive */
    int32_t walk_lds_stack;     /* -1 default (8) | stack entries per lane kept in LDS (0: all of them, one workgroup per CU) */
    int32_t walk_refill_min;    /* 0 default (24) | idle lanes of a wave that trigger k_walk's refill */
    int32_t walk_leaf_min;      /* 0 default (8) | lanes waiting at a leaf that trigger k_walk's triangle phase */
    int32_t walk_grid_mult;     /* 0 default (1) | k_walk's grid in resident sets of workgroups: each workgroup a contiguous 1/grid of the work list */
    int32_t quads_in_scan;      /* -1 auto | 0: a quad (two-triangle mesh: a lamp) beside meshes walked by k_walk sends the scene to the general scan kernels (inline mesh walk compiled in) */
    int32_t bounce_fit;         /* -1 auto | 0: k_bounce's general instance even where one compiled for the scene's feature set exists */
    int32_t plane_pairs;        /* -1 auto | 0: the flat scan's plane table holds single planes only (no two opposing planes share a division) */
} tinsel_hip_tuning;
enum { TINSEL_ACCUMULATE_AUTO = 0, TINSEL_ACCUMULATE_TILED = 1, TINSEL_ACCUMULATE_WIDE = 2, TINSEL_ACCUMULATE_PIPED = 3, TINSEL_ACCUMULATE_FULL_WINDOW = 4 };

/* Fills `t` with the defaults ("the library decides" everywhere). */
void tinsel_hip_tuning_init(tinsel_hip_tuning* t);
/* tinsel_hip_create with a tuning (NULL: the defaults, i.e. exactly tinsel_hip_create). */
tinsel_hip* tinsel_hip_create_tuned(const tinsel_scene_desc* scene, int device_index, const tinsel_hip_tuning* tuning);
/* The per-render fields of `tuning` from the next render on (the create-time fields are ignored: they are baked into the
 * uploaded scene).  Frees the path buffers (they are sized by grid_mult), drops any look-ahead. */
int tinsel_hip_set_tuning(tinsel_hip* r, const tinsel_hip_tuning* tuning);
/* The tuning in force (create-time fields as given to create, per-render fields as last set). */
int tinsel_hip_get_tuning(tinsel_hip* r, tinsel_hip_tuning* out);

/* Replaces GpuRenderer::~GpuRenderer (render.cu:1055-1068). */
void tinsel_hip_destroy(tinsel_hip* r);

/* Replaces GpuRenderer::Init (render.cu:1070-1075): (re)allocates and zeroes the
 * W*H float4 accumulation buffer. */
int tinsel_hip_init(tinsel_hip* r, int width, int height);

/* Same, but the accumulator is caller-owned DEVICE memory of W*H*4 floats (e.g. a
 * torch tensor, so the host language can hand it to RCCL); it is zeroed here and
 * must outlive the renderer or the next init. */
int tinsel_hip_init_external(tinsel_hip* r, int width, int height, float* device_accum);

/* Replaces GpuRenderer::Render (render.cu:1077-1103) with `passes` == 1: adds one
 * sample per pixel per pass to the device accumulator, then copies the running sum
 * (rgb*w, w) to `out_rgba` (W*H*4 floats, host memory).  `out_rgba` may be NULL
 * to skip the D2H copy (the accumulator stays resident in HBM). */
int tinsel_hip_render(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options,
                      float* out_rgba, int passes);

/* Look-ahead for callers that use tinsel_hip_render the way the reference's main loop does (main.cpp:246-250: one pass and
 * the full-frame running sum to the host per call, 16 calls per displayed frame).  With it on, a tinsel_hip_render call
 * returns as soon as ITS running sum has been copied out, and meanwhile the passes the next call will most probably ask
 * for (same camera, options and pass count) are traced into a second accumulator; a matching next call only swaps
 * buffers and copies, anything else drops the speculation.  Images are bit-identical to the plain path; the statistics
 * counters and tinsel_hip_read_batch_radiance see one call ahead (every other entry point drops the speculation first).
 * Off by default; the C++ shim turns it on (TINSEL_LOOKAHEAD_ON).
 * TINSEL_LOOKAHEAD_PIN_OUTPUT additionally page-locks the caller's output array IN PLACE (hipHostRegister) so that the
 * read-back is an asynchronous DMA: only for callers who guarantee that the array outlives the renderer, the next
 * tinsel_hip_init or the next tinsel_hip_set_lookahead -- the registration is dropped there, and registered memory must
 * not be freed before (the reference's own caller frees its array before Init, main.cpp:73-87: it gets plain ON). */
enum { TINSEL_LOOKAHEAD_OFF = 0, TINSEL_LOOKAHEAD_ON = 1, TINSEL_LOOKAHEAD_PIN_OUTPUT = 2 };
int tinsel_hip_set_lookahead(tinsel_hip* r, int enable);

/* Same, but never touches host memory: enqueues `passes` passes on `stream`
 * (a hipStream_t, may be NULL for the default stream) and returns without
 * synchronising.  Used by bench.py / multi-GPU hosts that own the stream. */
int tinsel_hip_render_async(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options,
                            int passes, void* stream);

/* Device pointer to the W*H*4 float accumulation buffer (for an RCCL reduce by the
 * host language, e.g. torch.distributed).  Valid until the next init/destroy. */
float* tinsel_hip_accum_device_ptr(tinsel_hip* r);

/* Blocking copy of the accumulator to host (W*H*4 floats). */
int tinsel_hip_read_accum(tinsel_hip* r, float* out_rgba);

/* Mesh BVHs.  TINSEL_BVH_REFERENCE (default): the trees the reference's host builder made (bvh.h:30-263), as
 * passed in tinsel_mesh_geometry::nodes -- the parity path, since a tree's visit order resolves exact-t ties.
 * TINSEL_BVH_LBVH: rebuild every mesh that does not live in LDS on the DEVICE (Morton-code linear BVH, one
 * triangle per leaf like the reference's trees; tn_lbvh.h) -- for meshes rebuilt per frame (main.cpp:318-327
 * re-inits per batch frame) or too large to wait for the host SAH sweep.  Same hits except exact ties; slower
 * to traverse than the SAH tree, far faster to build.  TINSEL_BVH_PLOC: the same, the hierarchy by parallel locally-ordered
 * clustering over the Morton order (agglomerative, surface-area driven: close to the SAH tree in render speed, a few ms to build).
 * *build_ms (may be NULL) receives the device build time. */
enum { TINSEL_BVH_REFERENCE = 0, TINSEL_BVH_LBVH = 1, TINSEL_BVH_PLOC = 2 };
int tinsel_hip_set_mesh_bvh(tinsel_hip* r, int mode, double* build_ms);

/* Refit for deforming meshes (per-frame vertex animation with unchanged topology; the reference rebuilds with its host SAH
 * sweep, mesh.cpp:314-338 -- 1.1 s for 524k triangles): `primitive`'s mesh gets new vertex positions (num_vertices x 3
 * floats, host; must be the vertex count the mesh was created with) and optionally new vertex normals (num_vertices x 3
 * floats, host; normals_xyz == NULL keeps the normals the mesh has); the triangle
 * records are re-gathered and every box of the mesh's CURRENT tree (the reference's, or a device-built one) is recomputed
 * bottom-up on the device -- exactly the boxes the reference's builder would store for that tree shape -- and, while a
 * device-built tree is in use, of the reference's tree too; the area CDF and PrimitiveArea of every instance follow
 * (Mesh::RebuildCDF's serial order), and so does the scene level: the leaf box of every instance is PrimitiveBounds under
 * the transforms in force, its ancestors the union of their children.  All instances of the mesh change.  A mesh small
 * enough for the LDS-staged arena is refitted like any other, in the arena's copy in HBM that every launch stages from. */
int tinsel_hip_refit_mesh(tinsel_hip* r, int primitive, const float* positions_xyz, int num_vertices, const float* normals_xyz);

/* Primitives that MOVE between renders, and the scene-level BVH that follows them.  The reference mutates Scene::primitives and
 * re-runs Scene::Build (scene.cpp:4-16: its host BVHBuilder over PrimitiveBounds(p), intersection.h:906-939), or re-loads an animated
 * scene file and re-creates the renderer per batch frame (main.cpp:318-327) -- re-uploading every mesh.  Here:
 *   tinsel_hip_set_primitive_transform   new start / end transforms of primitive `index` (the pose used by every intersection, the
 *       motion-blur interpolation when they differ, PrimitiveArea of a mesh light).  Takes effect with the next rebuild_scene: until
 *       then the renderer must not be asked to render.
 *   tinsel_hip_rebuild_scene             the scene BVH, the primitives' leaf boxes and the traversal stack depth, from PrimitiveBounds
 *       of the primitives as they are NOW.  TINSEL_SCENE_BVH_NODES: `nodes` (2P-1 reference-format nodes, e.g. the reference's own
 *       Scene::Build run on the host) is validated like at create and used as it is -- bit-identical to a renderer created from the moved
 *       scene.  TINSEL_SCENE_BVH_DEVICE: built on the device (the mesh builders' kernels, tn_lbvh.h: Morton order over the boxes'
 *       centroids, agglomerative clustering by surface area); nodes / num_nodes are ignored.  At the scene level the reference's
 *       QueryBVH has no closest-t cull (intersection.h:751-799), so the SET of primitives a ray tests does not depend on the tree:
 *       another tree changes the visit order only, which decides nothing but exact-t ties.  *build_ms (may be NULL): device time.
 * Meshes keep their own trees (tinsel_hip_refit_mesh / tinsel_hip_set_mesh_bvh for those). */
enum { TINSEL_SCENE_BVH_NODES = 0, TINSEL_SCENE_BVH_DEVICE = 1 };
int tinsel_hip_set_primitive_transform(tinsel_hip* r, int index, const tinsel_transform* start, const tinsel_transform* end);
int tinsel_hip_rebuild_scene(tinsel_hip* r, int mode, const tinsel_bvh_node* nodes, int num_nodes, double* build_ms);

/* Importance sampling of the environment probe.  TINSEL_PROBE_CDF (default): the reference's two binary searches over
 * the row and column CDFs (ProbeSample, probe.h:205-236; ~21 dependent loads per sample on the 1600x800 loft.hdr) --
 * sample-identical to the reference.  TINSEL_PROBE_ALIAS (opt-in): an alias table over the W*H texels built once on the
 * host from the same pdf tables; consumes the same two random numbers, draws texels with the same probabilities and
 * returns the same pdf for a texel, so the estimator is as unbiased -- but a given seed picks another texel, so images
 * agree with the reference's statistically, not sample for sample. */
enum { TINSEL_PROBE_CDF = 0, TINSEL_PROBE_ALIAS = 1 };
int tinsel_hip_set_probe_sampling(tinsel_hip* r, int mode);

/* Russian roulette, OPT-IN (start_bounce = 0, the default, is the reference's behaviour: render.cpp:250 runs every
 * path to maxDepth and so does the parity path).  With start_bounce = b > 0, after every bounce i >= b - 1 that has a
 * successor the path survives with probability q = min(1, max(throughput.rgb)) and its throughput is divided by q: the
 * estimate stays unbiased, deep low-throughput paths (glass at maxDepth 12) stop early.  Draws one extra number from
 * the path's stream when q < 1, so images differ from the reference's sample by sample; the same rule is restated in
 * the C oracle (port_set_russian_roulette) and the two are compared bit for bit. */
int tinsel_hip_set_russian_roulette(tinsel_hip* r, int start_bounce);

/* Resume a progressive render: replaces the accumulator with a saved one (W*H*4 floats, as read_accum returned
 * it) and sets the index of the next pass, so that `read_accum after k passes` + `write_accum(.., k)` + more passes
 * gives the same image bit for bit as one uninterrupted render (pass seeds depend on the pass index only). */
int tinsel_hip_write_accum(tinsel_hip* r, const float* rgba, uint32_t next_pass_index);

/* ---- display stage: what main.cpp does with the accumulator every frame (main.cpp:258-282) ----
 *
 * g_filtered[i] = LinearToSrgb(ToneMap(g_pixels[i]*(exposure/g_pixels[i].w), limit))   util.h:25-42, maths.h:1545-1555
 * and, when nlm_width != 0, NonLocalMeansFilter(g_filtered, g_exposed, W, H, nlm_falloff, nlm_width)  (nlm.cpp:35-77;
 * main.cpp:59-60 defaults: width 0 = off, falloff 200).  Runs on the device accumulator (the sum of all passes since
 * Init); options->mode != ePathTrace presents the raw accumulator, as the reference does.  The float image is
 * bit-identical to the host code's (same operation order; powf/expf as glibc 2.35 evaluates them).
 * out_rgba (W*H*4 floats, the array main.cpp hands to glDrawPixels / WritePng) may be NULL. */
int tinsel_hip_present(tinsel_hip* r, const tinsel_options* options, int nlm_width, float nlm_falloff, float* out_rgba);
int tinsel_hip_present_async(tinsel_hip* r, const tinsel_options* options, int nlm_width, float nlm_falloff, void* stream);
/* Device pointer to the most recently presented W*H*4 float image. */
const float* tinsel_hip_present_device_ptr(tinsel_hip* r);

/* WritePng's float -> 8-bit RGB conversion (png.cpp:323-343): x*255 + Randf + Randf - 0.5 from ONE default-seeded
 * serial Random stream over all pixels and channels, clamped and truncated.  Host code (the generator has no
 * skip-ahead); rgb receives W*H*3 bytes, top row first -- the payload of the PNG the reference writes. */
int tinsel_image_quantize_rgb8(const float* rgba, int width, int height, unsigned char* rgb);

/* Pixel-tile sharding for multi-GPU: this renderer traces only paths whose
 * generating pixel lies in a tile t with (t % world) == rank, tiles of
 * `tile`x`tile` pixels in raster order.  Seeds depend on (pixel, pass) only, so
 * the sum over ranks of the accumulators equals the world==1 image up to float
 * summation order.  Default: rank 0 of 1. */
int tinsel_hip_set_shard(tinsel_hip* r, int rank, int world, int tile);

int tinsel_hip_set_pipeline(tinsel_hip* r, int pipeline);

/* Arithmetic contract of the path kernels.
 * TINSEL_ARITH_EXACT (default, the parity path): no FMA contraction, IEEE divide / sqrt, glibc 2.35's sinf / cosf / expf
 *   restated -- every path bit-identical to the reference's CPU PathTrace on the same seeds.
 * TINSEL_ARITH_FAST (opt-in): the same kernels built the way the reference builds itself (`-O3 -ffast-math`, makefile:4;
 *   `-use_fast_math -prec-div=false -prec-sqrt=false`, tinsel.vcxproj:134): FMA contraction, v_rcp / v_rsq / v_sqrt,
 *   the hardware's sin / cos / exp.  Same seeds, same RNG streams; paths agree to rounding until a branch flips, and the
 *   image stays within the stated 1e-3 per-pixel L2 of the CPU reference at the spp the BASELINE configs use (measured by
 *   tests/test_gpu_fast.py and reported by bench.py as fast_l2).  Not bit-reproducible against the reference. */
enum { TINSEL_ARITH_EXACT = 0, TINSEL_ARITH_FAST = 1 };
int tinsel_hip_set_arithmetic(tinsel_hip* r, int mode);
int tinsel_hip_get_arithmetic(tinsel_hip* r);

/* The per-pass seed is the (pass_index+1)-th output of Random(1).Rand()
 * (mirrors `seed = Random(frame)` / `seed.Rand()`, render.cu:1050-1052,1099).
 * A new renderer starts at pass 0; Init does not reset it (nor does the reference). */
int tinsel_hip_set_pass_index(tinsel_hip* r, uint32_t pass_index);
uint32_t tinsel_hip_get_pass_index(tinsel_hip* r);

/* Counters since creation (or the last reset): rays = Trace()-equivalent casts
 * (extension + shadow; reference render.cpp:17 call sites :253,:122,:175),
 * samples = camera paths started, gpu_seconds = sum of HIP-event-timed spans. */
void tinsel_hip_stats(tinsel_hip* r, unsigned long long* rays, unsigned long long* samples,
                      double* gpu_seconds);
void tinsel_hip_reset_stats(tinsel_hip* r);

/* Per-kernel timing (HIP events on the launch stream) of the most recent
 * tinsel_hip_render* call, for bench.py's roofline block.  Returns the number
 * of kernel classes written (<= max_entries).  Blocks until the events resolve. */
typedef struct tinsel_kernel_time {
    char name[32];
    uint32_t launches;
    float total_ms;     /* sum of the launches' durations */
    float busy_ms;      /* union of their intervals: less than total_ms where a call's chunks overlap on two streams */
} tinsel_kernel_time;
int tinsel_hip_kernel_times(tinsel_hip* r, tinsel_kernel_time* out, int max_entries);
/* sizeof(tinsel_kernel_time) in THIS build of the library (40; 36 before busy_ms was added in round 4): a caller that may be handed an
 * older library (TINSEL_HIP_LIB) asks before it reads the records -- the symbol's absence says "36-byte records, no busy_ms". */
int tinsel_hip_kernel_time_bytes(void);
int tinsel_hip_enable_kernel_timing(tinsel_hip* r, int enable);

/* Extended counters since the last reset: [0]=rays [1]=samples [2]=internal BVH node visits
 * [3]=triangle tests [4]=primitive tests [5]=shadow rays [6..7] reserved.  [2..4] only advance
 * while detail counting is on (it costs a few percent); they feed B_ray of DESIGN.md. */
int tinsel_hip_stats_detail(tinsel_hip* r, unsigned long long* out8);
int tinsel_hip_set_detail_counters(tinsel_hip* r, int enable);

/* Per-pixel cost of path tracing passes [pass_begin, pass_begin + passes) as the reference algorithm counts it:
 * out[(j*W + i)*4 + {0,1,2,3}] = {rays, internal BVH node visits, triangle tests, primitive tests}, summed over the
 * passes (uint32, wraps). Pixels a shard does not own are 0. Leaves the accumulator, pass index, stats and tuning as they were.
 * rays = closest-hit and shadow rays; the four are the quantities of tinsel_hip_stats_detail's [0], [2], [3], [4], counted
 * on the scene BVH walk (never the flat scan), with the renderer's roulette, probe sampling and arithmetic.  Needs
 * options->mode == TINSEL_MODE_PATHTRACE and the frame size of the last tinsel_hip_init; kernel "k_cost" in
 * tinsel_hip_kernel_times. */
int tinsel_hip_render_cost(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options,
                           uint32_t pass_begin, int passes, uint32_t* out_host);

/* Feature buffers: the guide images a denoiser or a compositor takes beside the beauty -- albedo, shading normal, depth, coverage --
 * reconstructed EXACTLY as the beauty is.  For every path of the passes [pass_begin, pass_begin + passes) -- pass s at pixel (i, j): the
 * generator Random(i + j*W + pass_seed(pass_begin + s)), draws x, y, t, raster position (x + i, y + j), shutter time
 * Lerp(shutter_start, shutter_end, t): the beauty's own camera sample -- one closest-hit Trace() at that time gives per requested plane
 *   TINSEL_FEATURE_ALBEDO   the hit primitive's tinsel_material.color, bit for bit
 *   TINSEL_FEATURE_NORMAL   FaceForward(n, -direction): what tinsel_ray_hit carries for that ray
 *   TINSEL_FEATURE_DEPTH    (t, t*t, 1.0f), t*t one fp32 multiply
 * and (0, 0, 0) at a miss, and each plane is accumulated by AddSample's arithmetic (render.cpp:401-445) with options->filter at the path's
 * raster position: the same weights, in the same order, as the beauty's.  The clamp is +infinity; options->clamp, max_depth, exposure and
 * limit are ignored.  The albedo is the first surface's: specular surfaces are not looked through.
 * `out` holds popcount(features) planes of W*H float4 in ascending bit order, out[(p*H*W + j*W + i)*4 + c]: xyz the weighted sum, w the
 * weight sum, as in the accumulator; every plane starts from zero, so the call overwrites.  albedo = xyz/w; the mean normal is xyz/w,
 * renormalised by the caller; of DEPTH z/w is the coverage (alpha), x/z the mean depth over hits, y/z - (x/z)^2 its variance.
 * The seeds are a table of the call's own; the renderer's generator is only read.  The call respects the shard as a render does: a rank
 * generates the samples of the pixels it owns and adds them wherever their footprints reach, and the sum over the ranks is the whole
 * frame's planes up to fp32 summation order.  The scene is the one in force; tinsel_hip_set_arithmetic's arm traces the rays (the
 * accumulate stage is the same in both).  The accumulator, the pass index, the pass seeds, the statistics, the tuning, look-ahead and the
 * path buffers are left as they were, and tinsel_hip_stats does not count the call.  Kernels "k_features" (once per batch) and
 * "k_accumulate" (once per plane and batch) in tinsel_hip_kernel_times (with kernel timing on, the call starts a new record like a render).
 * Needs options->mode == TINSEL_MODE_PATHTRACE and the frame size of the last tinsel_hip_init.  Returns -1 and writes nothing for: a null
 * argument, passes < 1, features == 0 or features > 7, another mode, a frame size that does not match (or no tinsel_hip_init), a moved
 * primitive without tinsel_hip_rebuild_scene, and for the device entry an out_dev that is not 16-byte aligned.
 * Memory, kept until tinsel_hip_destroy: 16 bytes x popcount(features) per path slot of a batch -- a batch holds whole passes,
 * max(1, floor(batch_paths / slots per pass)) of them and no more than `passes`, a pass W*H slots (a shard: its own tiles); 1024 x 1024,
 * 16 passes, three planes: 768 MB -- plus 4 bytes per pass for the seeds, and for the host entry popcount(features)*W*H*16 bytes of planes.
 * Batches run one after the other and the result does not depend on the cut. */
#define TINSEL_FEATURE_ALBEDO 1u   /* bit 0 */
#define TINSEL_FEATURE_NORMAL 2u   /* bit 1 */
#define TINSEL_FEATURE_DEPTH  4u   /* bit 2 */

/* host array of popcount(features)*W*H*4 floats; returns when it is written */
int tinsel_hip_render_features(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options,
                               uint32_t pass_begin, int passes, unsigned features, float* out_host);
/* device array, 16-byte aligned; enqueued on `stream` (NULL: the default stream) and not waited for.  The call works in buffers of its own
 * and only reads the scene, like a ray query: it waits for nothing the renderer has in flight and nothing of the renderer's waits for it;
 * a later features call on another stream waits, on the device, for this one. */
int tinsel_hip_render_features_device(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options,
                                      uint32_t pass_begin, int passes, unsigned features, float* out_dev, void* stream);

/* ID mattes: which primitive is under each pixel, and by how much -- per pixel a ranked list of (id, filter-weight sum) pairs (Cryptomatte's
 * data model) on the beauty's own samples, so that a matte is anti-aliased, motion-blurred and filtered EXACTLY as the image is.  An id does
 * not average, so the feature planes above cannot carry it.
 * Samples and ids: every path of the passes [pass_begin, pass_begin + passes), with the camera sample and the shutter time of
 * tinsel_hip_render_features (generator Random(i + j*W + pass_seed(pass_begin + s)), draws x, y, t).  The id of a path is the primitive
 * index of its one closest-hit Trace() at that time -- what tinsel_ray_hit carries for that ray --, or TINSEL_ID_MISS where the path left
 * the scene.
 * Visiting order: a pixel visits its candidates in AddSample's order (render.cpp:401-445): passes ascending, within a pass the generating
 * pixels in raster order (rows ascending, columns ascending inside a row) -- the order in which the accumulator adds.
 * Which candidates count: the path generated at a pixel has the raster position (x + i, y + j) = (rx, ry) and the footprint
 * [max(0, int(rx - fw)), min(int(rx + fw), W - 1)] x [max(0, int(ry - fw)), min(int(ry + fw), H - 1)], fw = options->filter.width, as
 * AddSample's.  It is a candidate of every pixel (px, py) of its footprint, with the weight w = 1 for the box filter and, for the Gaussian,
 * w = G(px - rx)*G(py - ry) (one fp32 multiply), G(x) = max(0, expf(-falloff*x*x) - offset) as Filter::Gaussian.  A candidate with w == +0
 * is skipped entirely: it claims no slot and adds nothing (adding +0 to a non-negative sum changes no bit).
 * What a counting candidate (w > 0) does to its pixel, in this order:
 *   1. total += w;
 *   2. if one of the pixel's `slots` slots holds the id already: that slot's weight += w;
 *   3. otherwise, if a slot is empty: the FIRST empty slot takes (id, w);
 *   4. otherwise residual += w.
 * Every pixel starts from empty slots, residual = total = 0; all sums are fp32, one rounding per add.  Slots keep first-seen order from
 * batch to batch within a call, so the result does not depend on the batch cut.
 * Ranking: at the end of the call each pixel's slots are sorted: weight descending, ties by ascending id as int32, empty slots last.  An
 * occupied slot always has weight > 0; an empty one has id TINSEL_ID_EMPTY and weight 0.
 * Output, planar (pixel (i, j) of plane p at [(p*H + j)*W + i]): out_ids[slots][H][W] int32, the ranked ids; out_weights[slots + 2][H][W]
 * float, planes 0 .. slots - 1 the ranked slots' weights, plane `slots` the residual, plane `slots + 1` the total.  Both are overwritten.
 * The total plane is bit for bit the w of the accumulator, and of any tinsel_hip_render_features plane, for the same passes and filter.
 * A matte of a set of ids is (the sum of the weights of the slots that hold one of them)/total.
 * Everything else as tinsel_hip_render_features: the seeds are a table of the call's own and the renderer's generator is only read; the
 * accumulator, the pass index, the pass seeds, the statistics, the tuning, look-ahead and the path buffers are left as they were, and
 * tinsel_hip_stats does not count the call; tinsel_hip_set_arithmetic's arm traces the rays (the lists are built the same way in both);
 * options->clamp, max_depth, exposure and limit are ignored.  Under a shard a rank processes the samples of the pixels it owns wherever
 * their footprints reach: the result is that rank's PARTIAL list, and merging the ranks' lists (sum the weights of equal ids, re-rank, add
 * what no longer fits to the residual, sum residuals and totals: tinsel_amd.merge_id_mattes) is the caller's job.
 * Kernels: "k_ids" (once per batch) is timed under the name "k_features" in tinsel_hip_kernel_times -- the name table does not grow --,
 * and the gather ("k_ids_accumulate", once per batch) and the ranking ("k_ids_rank", once per call) have no class there, like the denoise
 * stage's kernels: time the device entry with events on the stream it is given (profiles/id_mattes_measure.py).
 * Needs options->mode == TINSEL_MODE_PATHTRACE and the frame size of the last tinsel_hip_init.  Returns -1 and writes nothing for: a null
 * argument, passes < 1, slots outside 1 .. TINSEL_ID_MAX_SLOTS, another mode, a frame size that does not match (or no tinsel_hip_init), a
 * moved primitive without tinsel_hip_rebuild_scene, and for the device entry a pointer that is not 16-byte aligned (or buffers that overlap).
 * Memory, kept until tinsel_hip_destroy: 4 bytes per path slot of a batch -- a batch holds whole passes, max(1, floor(batch_paths / slots
 * per pass)) of them and no more than `passes`, a pass W*H slots (a shard: its own tiles); 1024 x 1024, 16 passes: 64 MB --, 72 bytes per
 * pixel for the lists between batches (eight ids, eight weights, residual, total, whatever `slots` is), 4 bytes per pass for the seeds,
 * and for the host entry (8*slots + 8)*W*H bytes of ranked planes. */
#define TINSEL_ID_MISS   (-1)   /* the path left the scene */
#define TINSEL_ID_EMPTY  (-2)   /* an unused slot */
#define TINSEL_ID_MAX_SLOTS 8

/* host arrays of slots*W*H int32 and (slots + 2)*W*H floats; returns when they are written */
int tinsel_hip_render_id_mattes(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options,
                                uint32_t pass_begin, int passes, int slots, int32_t* out_ids_host, float* out_weights_host);
/* device arrays, each 16-byte aligned; enqueued on `stream` (NULL: the default stream) and not waited for, under the stream and fence rules
 * of tinsel_hip_render_features_device: the call waits for nothing the renderer has in flight and nothing of the renderer's waits for it;
 * a later ID-matte call on another stream waits, on the device, for this one. */
int tinsel_hip_render_id_mattes_device(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options,
                                       uint32_t pass_begin, int passes, int slots, int32_t* out_ids_dev, float* out_weights_dev, void* stream);

/* Light groups: the beauty split by which emitter produced it, in ONE trace of the paths -- lights can be re-balanced, tinted or switched
 * off in comp without another render.  The integrator is linear in emission: every term it adds to a path's radiance is a product with
 * exactly one emitter's colour -- the primitive whose `emission` is read (a camera ray or a BSDF ray that hits it; the primitive a light
 * sample's shadow ray ENDS on, which need not be the light that was sampled), or the sky / probe (a ray that leaves the scene, the probe's
 * light sample) -- and emission never steers a path.  So each term is deposited into the plane of its emitter's group.
 * Plane g is DEFINED as the accumulator tinsel_hip_render would produce for the passes [pass_begin, pass_begin + passes) on the same scene
 * with emission = 0 on every primitive i whose group_of_primitive[i] != g and sky horizon = zenith = 0 unless env_group == g: bit for bit
 * in all four channels wherever that render is finite.  It follows that
 *   - options->clamp applies to EACH PLANE SEPARATELY (ClampLength is not linear): the planes add up to the beauty, within fp32 rounding,
 *     only with clamp = FLT_MAX;
 *   - the weight channel of every plane is the beauty's;
 *   - a primitive with emission but light_samples == 0 (found by BSDF rays only) has its group like any light.
 * A PROBE is not masked by the definition (it shapes light sampling and MIS in every plane): its radiance lands in env_group only, the
 * env_group plane is the render with every emission zeroed, and a light's plane is (the render masked to that group) - (the env_group
 * plane) up to fp32 rounding.
 * group_of_primitive: num_primitives int32, the group of each primitive of the scene in force, -1: in no group (its emission reaches no
 * plane); env_group likewise for the sky / probe.  `out` holds num_groups planes of W*H float4, out[(g*H*W + j*W + i)*4 + c], every plane
 * from zero: the call overwrites.
 * The call traces the camera's paths through the split pipeline whatever tinsel_hip_set_pipeline says (k_generate, k_extend, k_lights,
 * k_shadow and the walk and segment kernels as a render plans them; the shading kernel is k_shade_groups, timed under the name "k_shade" in
 * tinsel_hip_kernel_times -- the name table does not grow), then one "k_accumulate" per plane and batch.  The seeds, the planes' records
 * and the statistics the kernels count into are the call's own: the accumulator, the pass index, the renderer's seed table and
 * tinsel_hip_stats are left as they were, and a render, a light-groups call and the render that follows give the images of the two renders
 * alone.  The paths themselves live in the renderer's path buffers, used under the fences of the radiance queries.
 * options->max_depth < 1 gives all-zero planes.  Returns -1 before anything is launched or written for: a null argument, passes < 1,
 * num_groups outside 1 .. TINSEL_MAX_LIGHT_GROUPS, env_group or a table entry outside -1 .. num_groups - 1, another mode than
 * TINSEL_MODE_PATHTRACE, a frame size that does not match the last tinsel_hip_init, a moved primitive without tinsel_hip_rebuild_scene, a
 * sharded renderer (world > 1), TINSEL_ARITH_FAST, and for the device entry an out_dev that is not 16-byte aligned.
 * Memory, kept until tinsel_hip_destroy: 16 bytes x num_groups per path slot of a batch -- a batch holds whole passes, and those bytes count
 * against batch_paths beside the 176 bytes of a path's own state: max(1, floor(batch_paths*176/(176 + 16*num_groups) / (W*H))) passes --
 * plus 4 bytes per pass for the seeds, one byte per primitive for the table, and for the host entry num_groups*W*H*16 bytes of planes. */
#define TINSEL_MAX_LIGHT_GROUPS 8

/* host array of num_groups*W*H*4 floats; returns when it is written */
int tinsel_hip_render_light_groups(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options,
                                   uint32_t pass_begin, int passes, int num_groups, const int32_t* group_of_primitive, int env_group,
                                   float* out_host);
/* device array, 16-byte aligned; enqueued on `stream` (NULL: the default stream) and not waited for; the table is a HOST array, read before
 * the call returns.  The stream waits, on the device, for what the renderer's path buffers still serve and for an earlier light-groups call
 * on another stream. */
int tinsel_hip_render_light_groups_device(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options,
                                          uint32_t pass_begin, int passes, int num_groups, const int32_t* group_of_primitive, int env_group,
                                          float* out_dev, void* stream);

/* Depth planes: the beauty at SEVERAL PATH DEPTHS in one trace of the paths -- direct and indirect light for the compositor and the
 * denoiser (indirect light is the noisy part and takes the stronger filter), and what every further bounce adds for whoever picks
 * max_depth, without one render per depth that retraces the bounces before it.  The integrator adds to a path's radiance bounce by bounce,
 * and nothing it draws or decides at bounce i depends on max_depth except that the loop stops: a path's radiance after the iteration
 * i = d - 1 IS PathTrace(..., maxDepth = d).
 * Plane k of `out`, out[((k*H + j)*W + i)*4 + c], is DEFINED as the accumulator tinsel_hip_render gives from a zeroed accumulator at pass
 * index pass_begin after `passes` passes with options->max_depth replaced by depths[k]: bit for bit in all four channels, the weight
 * included, wherever that render is finite.  It follows that
 *   - options->max_depth is not read: the trace runs to depths[num_planes - 1];
 *   - options->clamp applies to EACH PLANE SEPARATELY (ClampLength is applied per sample): with a finite clamp a deeper plane's colour may
 *     be below a shallower one's; with clamp = FLT_MAX the colour never decreases from plane to plane (every term is non-negative);
 *   - the renderer's Russian-roulette setting applies: roulette after bounce b changes only what comes later;
 *   - the weight channel of every plane is the beauty's.
 * depths: a HOST array of num_planes int32, strictly ascending, 1 <= depths[0], depths[num_planes - 1] <= TINSEL_MAX_PLANE_DEPTH; read
 * before the call returns.  flags: TINSEL_DEPTH_PLANES_ADD adds the passes to what `out` holds instead of starting every plane from zero --
 * the passes [0, a) followed by [a, b) with the flag equal [0, b) in one call, bit for bit; TINSEL_DEPTH_PLANES_ACCUMULATE_SINGLY adds every
 * plane's batch with a launch of the render's own accumulate kernels instead of one launch for all planes of a batch (the same bits; the
 * A/B arm, and what filters wider than 2 take anyway).
 * The call traces the camera's paths through the split pipeline whatever tinsel_hip_set_pipeline says (k_generate, k_extend, k_lights,
 * k_shadow and the walk and segment kernels as a render plans them; the shading kernel is k_shade_depths, timed under the name "k_shade" in
 * tinsel_hip_kernel_times -- the name table does not grow): at the end of a bounce's shading the path's own lane writes its radiance, one
 * 16-byte record, into the plane whose depth that bounce completes, and a path that ends early into every deeper plane too, so every
 * (path, plane) record is written exactly once.  Then one "k_accumulate" per batch (k_views_accumulate, the planes as its second grid
 * dimension) or per plane and batch.  The seeds, the planes' records and the statistics the kernels count into are the call's own: the
 * accumulator, the pass index, the renderer's seed table and tinsel_hip_stats are left as they were, and a render, a depth-planes call and
 * the render that follows give the images of the two renders alone.  The paths themselves live in the renderer's path buffers, used under
 * the fences of the radiance queries.
 * Returns -1 before anything is launched or written for: a null argument, passes < 1, num_planes outside 1 .. TINSEL_MAX_DEPTH_PLANES, a
 * depths array that is not strictly ascending inside 1 .. TINSEL_MAX_PLANE_DEPTH, unknown flag bits, another mode than
 * TINSEL_MODE_PATHTRACE, a frame size that does not match the last tinsel_hip_init, a moved primitive without tinsel_hip_rebuild_scene, a
 * sharded renderer (world > 1), TINSEL_ARITH_FAST (the contract is a bit contract), and for the device entry an out_dev that is not
 * 16-byte aligned.
 * Memory, kept until tinsel_hip_destroy: 16 bytes x num_planes per path slot of a batch -- a batch holds whole passes, and those bytes count
 * against batch_paths beside the 176 bytes of a path's own state: max(1, floor(batch_paths*176/(176 + 16*num_planes) / (W*H))) passes --
 * plus 4 bytes per pass for the seeds, and for the host entry num_planes*W*H*16 bytes of planes. */
#define TINSEL_MAX_DEPTH_PLANES 16
#define TINSEL_MAX_PLANE_DEPTH  64
#define TINSEL_DEPTH_PLANES_ADD                1   /* add to what `out` holds instead of starting every plane from zero */
#define TINSEL_DEPTH_PLANES_ACCUMULATE_SINGLY  2   /* one launch of the render's own accumulate kernels per plane (the A/B arm and the fallback) */

/* host array of num_planes*W*H*4 floats (read first with TINSEL_DEPTH_PLANES_ADD); returns when it is written */
int tinsel_hip_render_depth_planes(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options,
                                   uint32_t pass_begin, int passes, int num_planes, const int32_t* depths, int flags,
                                   float* out_host);
/* device array, 16-byte aligned; enqueued on `stream` (NULL: the default stream) and not waited for.  The stream waits, on the device, for
 * what the renderer's path buffers still serve and for an earlier depth-planes call on another stream. */
int tinsel_hip_render_depth_planes_device(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options,
                                          uint32_t pass_begin, int passes, int num_planes, const int32_t* depths, int flags,
                                          float* out_dev, void* stream);

/* View batches: the frames of MANY cameras on the one resident scene in one call -- the faces of a cube map, a stereo pair, a turntable,
 * a few hundred small views as a training set -- where a loop over tinsel_hip_set_pass_index and tinsel_hip_render pays every launch of
 * every bounce and an accumulate launch of a few tiles once per view.
 * Plane v of `out`, out[((v*H + j)*W + i)*4 + c], is DEFINED as the accumulator tinsel_hip_render gives for cameras[v] from a zeroed
 * accumulator at pass index pass_begin after `passes` passes: bit for bit in all four channels, the weight included.  All views share one
 * seed table, pass_seed(pass_begin + s) for s in [0, passes); the path of (view v, pass s, pixel i, j) is the camera sample of cameras[v]
 * seeded with i + j*W + pass_seed(pass_begin + s), traced with options->max_depth and the renderer's Russian-roulette setting, and added
 * with options->filter and options->clamp by AddSample's rule, each pixel's adds in pass order, then raster order of the generating pixels.
 * flags: TINSEL_VIEWS_ADD adds to what `out` holds instead of starting every plane from zero -- the passes [0, a) followed by [a, b) with
 * the flag equal [0, b) in one call, bit for bit; TINSEL_VIEWS_ACCUMULATE_SINGLY adds every view's batch with a launch of the render's own
 * accumulate kernels instead of one launch for all views of a batch (the same bits; the A/B arm, and what filters wider than 2 take anyway).
 * The paths run the split or the paired pipeline, as a radiance query's do, also on a scene a render takes through the fused kernel and
 * under every tinsel_hip_set_pipeline setting: k_generate_views in the place of k_generate -- timed under the name "k_generate" in
 * tinsel_hip_kernel_times, the name table does not grow --, then one "k_accumulate" per batch (k_views_accumulate) or per view and batch.
 * A batch is a run of consecutive views times a run of consecutive passes, as tinsel_hip_plan_views states it for the renderer's
 * batch_paths; each pixel's adds stay in pass order, so the cut shows nowhere.
 * The seeds, the cameras' table, the batch's radiance and the statistics the kernels count into are the call's own: the accumulator, the
 * pass index, the renderer's seed table, tinsel_hip_stats, the tuning and look-ahead work in flight are left as they were, and a render, a
 * views call and the render that follows give the images of the two renders alone.  The paths themselves live in the renderer's path
 * buffers, used under the fences of the radiance queries.  A scene with moved or refitted primitives is served as radiance queries serve it
 * (after tinsel_hip_rebuild_scene).  A group has no entry.
 * options->max_depth < 1 zeroes the planes (with TINSEL_VIEWS_ADD: leaves them untouched).  Returns -1 before anything is launched or
 * written for: a null argument, num_views outside 1 .. TINSEL_MAX_VIEWS, passes < 1 (or so many that a view's slots passes*W*H reach 2^32 -
 * 1), another mode than TINSEL_MODE_PATHTRACE, a frame size that does not match the last tinsel_hip_init, a moved primitive without
 * tinsel_hip_rebuild_scene, a sharded renderer (world > 1), TINSEL_ARITH_FAST (the contract is a bit contract), unknown flag bits, and
 * for the device entry an out_dev that is not 16-byte aligned.
 * Memory, kept until tinsel_hip_destroy: 16 bytes per path slot of a batch, 96 bytes per view, 4 bytes per pass, and for the host entry
 * num_views*W*H*16 bytes of planes. */
#define TINSEL_MAX_VIEWS 4096
#define TINSEL_VIEWS_ADD               1u  /* add to what `out` holds instead of starting every plane from zero */
#define TINSEL_VIEWS_ACCUMULATE_SINGLY 2u  /* one launch of the existing accumulate kernels per view (the A/B arm and the fallback) */

/* host array of num_views*W*H*4 floats (read first with TINSEL_VIEWS_ADD); returns when it is written */
int tinsel_hip_render_views(tinsel_hip* r, const tinsel_camera* cameras, int num_views, const tinsel_options* options,
                            uint32_t pass_begin, int passes, unsigned flags, float* out_rgba_host);
/* device array, 16-byte aligned; enqueued on `stream` (NULL: the default stream) and not waited for; the cameras are a HOST array, read
 * before the call returns.  The stream waits, on the device, for what the renderer's path buffers still serve and for an earlier views
 * call on another stream. */
int tinsel_hip_render_views_device(tinsel_hip* r, const tinsel_camera* cameras, int num_views, const tinsel_options* options,
                                   uint32_t pass_begin, int passes, unsigned flags, float* out_rgba_dev, void* stream);
/* The batch cut of a views call, host arithmetic only (no GPU needed): out3 = { views per batch, passes per batch, batches } for a limit
 * of slot_limit path slots per batch (the renderer's batch_paths).  If one view's passes fit -- passes*W*H <= slot_limit -- a batch takes
 * min(num_views, floor(slot_limit/(passes*W*H))) whole views with all their passes, the last batch the remainder; otherwise a batch takes
 * ONE view with min(passes, max(1, floor(slot_limit/(W*H)))) passes.  There is always at least one pass of one view per batch, however
 * small the limit.  Returns -1 for a bad argument and where a batch would have 2^32 - 1 slots or more. */
int tinsel_hip_plan_views(unsigned long long slot_limit, int width, int height, int passes, int num_views, int* out3);

/* Sample maps: a per-pixel pass count in one call -- a crop or region re-render whose pixels equal the full frame's, more samples where
 * the image is still noisy and none where it has converged, foveated budgets, the few pixels around a firefly -- where every other entry
 * traces whole frames, passes x W x H paths.  The entry is the mechanism only: the caller says how many passes each pixel gets; statistics,
 * error estimates and stopping rules live in the caller's code on top of it.
 * SAMPLES TRACED.  Pixel q = (i, j) gets the samples of levels t = 0 .. counts[j*W + i] - 1.  The sample of (q, t) is exactly the path a
 * render starts for pixel q in pass pass_begin + t: its camera sample is seeded i + j*W + pass_seed(pass_begin + t), and it is traced with
 * options->max_depth and the renderer's Russian-roulette setting.
 * HOW THEY ARE ADDED.  out[H][W][4] starts from zero, or with TINSEL_SAMPLES_ADD from what it holds, and receives AddSample of exactly
 * those samples with options->filter and options->clamp, each receiving pixel's adds in level order, then in raster order of the
 * generating pixels.  A sample that does not exist is skipped -- it is not added as zero: the weight channel does not see it.
 * WHAT FOLLOWS.  A uniform map n gives the accumulator of n passes from zero at pass_begin, bit for bit (tinsel_hip_render_views with this
 * one camera).  A uniform call of a passes followed by a map c at pass_begin + a with TINSEL_SAMPLES_ADD equals the single map a + c at
 * pass_begin.  An all-zero map zeroes `out` (with the flag: leaves it untouched); so does options->max_depth < 1.
 * The counts are a HOST array in both entries, read before the call returns (a device-resident map is not offered).
 * The paths run the split or the paired pipeline, as a radiance query's do, under every tinsel_hip_set_pipeline setting:
 * k_generate_samples in the place of k_generate -- timed under the name "k_generate" in tinsel_hip_kernel_times --, then one
 * "k_accumulate" per batch (k_samples_accumulate), whose tiles run to the largest count among their own candidates and no further.  A
 * batch is a run of consecutive levels, as tinsel_hip_plan_sample_map states it for the renderer's batch_paths; within a batch the slot
 * of (q, t) is the number of samples of the pixels before q plus t - t0 (pixel-major, compact).  Every pixel's adds stay in level order
 * across batches, so the cut shows nowhere.
 * The seeds, offsets, radiance and statistics are the call's own: the accumulator, the pass index, the renderer's seed table,
 * tinsel_hip_stats, the tuning and look-ahead work in flight are left as they were, and a render, a sample-map call and the render that
 * follows give the images of the two renders alone.  A group has no entry.
 * Returns -1 before anything is launched or written for: a null argument, another mode than TINSEL_MODE_PATHTRACE, a frame size that does
 * not match the last tinsel_hip_init, a sharded renderer (world > 1), TINSEL_ARITH_FAST (the contract is a bit contract), a moved
 * primitive without tinsel_hip_rebuild_scene, unknown flag bits, for the device entry an out_dev that is not 16-byte aligned, a batch of
 * 2^32 - 1 slots or more, and a filter whose footprint the tiled accumulate kernels do not hold (widths above 2: there is no untiled
 * masked accumulate kernel, and the error text says so).
 * Memory, kept until tinsel_hip_destroy: 16 bytes per path of a batch, 4 bytes per pixel (the offsets), 4 bytes per level (the
 * seeds), and for the host entry W*H*16 bytes of plane. */
#define TINSEL_SAMPLE_MAP_MAX 65535     /* the largest count of a pixel: what a uint16_t holds */
#define TINSEL_SAMPLES_ADD 1u           /* add to what `out` holds instead of starting from zero */

/* host array of W*H*4 floats (read first with TINSEL_SAMPLES_ADD); returns when it is written */
int tinsel_hip_render_sample_map(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options,
                                 uint32_t pass_begin, const uint16_t* counts, unsigned flags, float* out_rgba_host);
/* device array, 16-byte aligned; enqueued on `stream` (NULL: the default stream) and not waited for -- except between the batches of a
 * map that needs several: each batch's offsets are uploaded when the batch before has run.  The stream waits, on the device, for what
 * the renderer's path buffers still serve. */
int tinsel_hip_render_sample_map_device(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options,
                                        uint32_t pass_begin, const uint16_t* counts, unsigned flags, float* out_rgba_dev, void* stream);
/* The batch cut of a sample-map call, host arithmetic only (no GPU needed): out4 = { levels per batch, batches, total paths, largest
 * count } for a limit of slot_limit path slots per batch (the renderer's batch_paths).  Levels are cut into runs of
 * L = max(1, floor(min(slot_limit, 2^32 - 2)/(W*H))) consecutive levels -- a bound that needs no histogram of the map --, batches =
 * ceil(largest count / L); the batch [t0, t0 + L) holds sum over q of clamp(counts[q] - t0, 0, L) paths.  Returns -1 for a bad argument
 * and where one level, W*H slots, would reach 2^32 - 1 (the counts are not read then). */
int tinsel_hip_plan_sample_map(unsigned long long slot_limit, int width, int height, const uint16_t* counts, unsigned long long* out4);

/* Feature-guided denoise: a joint non-local-means filter on LINEAR radiance, in front of the display stage, guided by the planes above.
 * With features == 0 and demodulate == 0 it is NonLocalMeansFilter (nlm.cpp:35-77) on the normalised colour, bit for bit, falloff =
 * k_color and AverageFilter's radius = patch_radius; the guide terms add to the exponent.  Everything is fp32, one rounding per
 * operation (no FMA), IEEE divide, expf as glibc 2.35 evaluates it; tinsel_hip_set_arithmetic does not change the stage.
 * Inputs, all W*H float4 in accumulator form: the beauty B (xyz the sum, w the weight) and popcount(features) planes in ascending bit
 * order -- the layout tinsel_hip_render_features returns: A albedo, N normal, D depth.
 * Prepare, per pixel p: colour c = B.xyz/B.w (0 where B.w == 0), albedo a = A.xyz/A.w, normal n = N.xyz/N.w (the mean normal, not
 *   renormalised), depth z = D.x/D.z -- each 0 where its divisor is 0 or its plane is absent.  With demodulate: d_k = (a_k < albedo_floor)
 *   ? albedo_floor : a_k and u_k = c_k/d_k; without: u = c, d = 1.  U = (u, 0).
 * Means: M = AverageFilter(U, patch_radius) (nlm.cpp:4-33).
 * Filter, per pixel p, over the window of `radius` clipped to the frame, fx ascending outside, fy ascending inside, tap q:
 *   e = k_color*LengthSq(M_p - M_q)                                         (dx*dx + dy*dy + dz*dz + dw*dw, left to right)
 *   ALBEDO: e = e + k_albedo*LengthSq(a_p - a_q)     NORMAL: e = e + k_normal*LengthSq(n_p - n_q)           (three components each)
 *   DEPTH:  den = z_p*z_p + z_q*z_q, dz = z_p - z_q, e = e + k_depth*((den != 0) ? dz*dz/den : 0)
 *   weight = expf(-e); sum_k += u_q,k*weight; total += weight               (the term of an absent plane is skipped)
 * Output: (sum_k*(1.0f/total))*d_p,k in xyz and 1.0f in w: denoised radiance as an accumulator of weight one, which
 *   tinsel_hip_present_image_device takes.  A pixel with B.w == 0 takes part with colour 0.
 * The stage is meant for a WHOLE frame: a shard's accumulator holds its own tiles only -- reduce across the ranks first
 * (tinsel_hip_comm_reduce_accum, or a group's reduced frame) and denoise the sum.
 * beauty == NULL is the renderer's own accumulator; width and height must then be those of the last tinsel_hip_init.  planes may be
 * NULL only when features == 0.  The stage works in buffers of its own, owned by the renderer and kept until tinsel_hip_destroy (four
 * W*H float4 images, and for the host entry the inputs and the output); it leaves the accumulator, the pass index, the statistics, the
 * tuning and look-ahead as they were.  Returns -1 and writes nothing for: a null argument, a parameter out of range, features > 7,
 * demodulate without TINSEL_FEATURE_ALBEDO, a non-positive size, for the device entry a pointer that is not 16-byte aligned, and
 * beauty == NULL without a tinsel_hip_init or with another size.
 * Timing: the stage's kernels (k_denoise_prepare, k_nlm_means, k_denoise) have no class in tinsel_hip_kernel_times; time the device
 * entry with events on the stream it is given (profiles/denoise_measure.py). */
typedef struct tinsel_hip_denoise_params {   /* 32 bytes */
    int radius;                     /* 1 .. 8: the search window */
    int patch_radius;               /* 0 .. 4: AverageFilter's radius */
    float k_color, k_albedo, k_normal, k_depth;   /* finite, >= 0 */
    int demodulate;                 /* 0 | 1; 1 needs TINSEL_FEATURE_ALBEDO */
    float albedo_floor;             /* finite, > 0 */
} tinsel_hip_denoise_params;

/* the defaults (profiles/denoise_defaults.md) */
void tinsel_hip_denoise_params_init(tinsel_hip_denoise_params* p);

/* host arrays; returns when out_host (W*H*4 floats) is written */
int tinsel_hip_denoise(tinsel_hip* r, const float* beauty_host, const float* planes_host,
                       unsigned features, int width, int height,
                       const tinsel_hip_denoise_params* p, float* out_host);
/* device arrays, 16-byte aligned; enqueued on `stream` (NULL: the default stream) and not waited for, as tinsel_hip_render_features_device:
 * the call waits for nothing the renderer has in flight -- with beauty_dev == NULL the caller orders it behind the render, as with
 * tinsel_hip_present_async -- and a later denoise call on another stream waits, on the device, for this one.  Every input is read by
 * the first kernel and out_dev written by the last: out_dev may be one of the inputs. */
int tinsel_hip_denoise_device(tinsel_hip* r, const float* beauty_dev, const float* planes_dev,
                              unsigned features, int width, int height,
                              const tinsel_hip_denoise_params* p, float* out_dev, void* stream);

/* tinsel_hip_present_async with the source made an argument: any accumulator-form image of the init size on the device, 16-byte
 * aligned -- the denoised image, a reduced frame.  tinsel_hip_present_async is this call with the renderer's accumulator;
 * tinsel_hip_present_device_ptr names the result of either. */
int tinsel_hip_present_image_device(tinsel_hip* r, const float* image_dev,
                                    const tinsel_options* options, int nlm_width,
                                    float nlm_falloff, void* stream);

/* Ray queries on the resident scene: the reference's Trace() (render.cpp:17-62) for rays the caller chooses.
 * TINSEL_QUERY_CLOSEST: the smallest t > 0 over the primitives the ray reaches (an exact tie: the one the scene BVH walk meets first),
 * that primitive's index and its normal turned towards the ray, FaceForward(n, -direction); a miss is t = FLT_MAX, primitive = -1,
 * normal (0, 0, 0); tmax is ignored.  TINSEL_QUERY_OCCLUDED: 1 iff some primitive gives 0 < t < tmax (strict; tmax = +inf: any hit;
 * NaN or non-positive: never).  `time` is the pose of moving primitives, as a path's shutter time; `direction` is used as given.
 * The scene is the one in force (rebuild_scene, refit_mesh, set_mesh_bvh, set_arithmetic).  A query leaves the accumulator, pass index,
 * statistics, tuning, look-ahead and shard as they were, needs no tinsel_hip_init and ignores the shard; kernel "k_query" in
 * tinsel_hip_kernel_times (with kernel timing on, a query starts a new record like a render call does: the spans of the call before it
 * are dropped).  Bad arguments return -1 and launch nothing.  The host entries keep their staging buffers until tinsel_hip_destroy:
 * at most 64 MB for tinsel_hip_trace_rays, width*height*32 bytes up to 128 MB for tinsel_hip_trace_camera (larger frames go in several launches). */
typedef struct tinsel_ray     { float ox, oy, oz, time;  float dx, dy, dz, tmax; } tinsel_ray;
typedef struct tinsel_ray_hit { float t; int32_t primitive; float nx, ny, nz; uint32_t reserved[3]; } tinsel_ray_hit;

#define TINSEL_QUERY_CLOSEST  0   /* out: tinsel_ray_hit[n] */
#define TINSEL_QUERY_OCCLUDED 1   /* out: uint32_t[n], 1 or 0 */

/* host arrays, any 0 <= n <= 2^31 - 1 (staged through device buffers the renderer keeps, in chunks); returns when `out_host` is written */
int tinsel_hip_trace_rays(tinsel_hip* r, int mode, long long n, const tinsel_ray* rays_host, void* out_host);
/* device arrays, 16-byte aligned, not overlapping; enqueued on `stream` (NULL: the default stream, where the renderer works), not waited for */
int tinsel_hip_trace_rays_device(tinsel_hip* r, int mode, long long n, const tinsel_ray* rays_dev, void* out_dev, void* stream);
/* TINSEL_QUERY_CLOSEST of GenerateRay(i, j) for every pixel of a width x height frame (raster x = i, y = j, no jitter: the rays of
 * TINSEL_MODE_NORMALS), generated on the device; out_host[j*width + i] */
int tinsel_hip_trace_camera(tinsel_hip* r, const tinsel_camera* camera, int width, int height, float time, tinsel_ray_hit* out_host);

/* Radiance queries on the resident scene: the reference's PathTrace(scene, origin, dir, time, maxDepth, rand) (render.cpp:230-388) for
 * paths the caller starts -- light-map and probe baking, radiance caches, re-tracing one pixel's samples, reference radiance for rays in
 * a device tensor.  One record starts one path: the ray (`direction` is used as given; PathTrace expects unit length), the shutter time
 * that poses moving primitives, and rng1 / rng2, the two words of the reference's Random at the moment PathTrace is entered -- for
 * Random(seed): rng1 = 315645664 + seed, rng2 = rng1 ^ 0x13ab45fe.  Reserved words are ignored.  A caller who wants many samples of one
 * ray repeats it with different generator words.
 * out[4*k .. 4*k + 2] is the value PathTrace returns for record k, bit for bit under TINSEL_ARITH_EXACT: unclamped and unfiltered (clamp
 * and the reconstruction filter belong to AddSample, which a query does not run); out[4*k + 3] is reserved.
 * A query uses the scene in force (rebuild_scene, refit_mesh, set_mesh_bvh) and the renderer's roulette, probe-sampling and arithmetic
 * settings; it ignores the shard, needs no tinsel_hip_init, and leaves the accumulator, the pass index, the pass seeds, the tuning and
 * look-ahead as they were.  Its rays and samples ARE counted in tinsel_hip_stats: a query is path tracing.  It runs the paired
 * pipeline where a render would and the split pipeline otherwise (also under TINSEL_PIPELINE_MEGAKERNEL and on scenes a render takes
 * through the fused kernel), behind kernel "k_generate_rays" in tinsel_hip_kernel_times (with kernel timing on, a query starts a new
 * record like a render call does).  More paths than tinsel_hip_set_batch_paths allows run as several batches, one after the other;
 * the result does not depend on the cut.  Bad arguments -- a null renderer, n < 0 or n >= 2^31, max_depth < 1, a null array with n > 0,
 * a moved primitive without tinsel_hip_rebuild_scene -- return -1 and launch nothing; n == 0 returns 0.
 * Memory: the paths are traced in the renderer's path buffers, the state of min(n, batch_paths) paths (a render that runs another
 * pipeline allocates its own again); the host entry adds staging buffers kept until tinsel_hip_destroy, shared with
 * tinsel_hip_trace_rays: at most 64 MB (2^20 paths per chunk: 48 MB of records, 16 MB of results), whatever n is. */
typedef struct tinsel_path_start { float ox, oy, oz, time;  float dx, dy, dz, reserved0;  uint32_t rng1, rng2, reserved1, reserved2; } tinsel_path_start;

/* host arrays (staged through device buffers the renderer keeps, in chunks); returns when `out_rgbx_host` is written */
int tinsel_hip_trace_radiance(tinsel_hip* r, long long n, const tinsel_path_start* starts_host, int max_depth, float* out_rgbx_host);
/* device arrays, 16-byte aligned, not overlapping; enqueued on `stream` (NULL: the default stream) and not waited for.  The path buffers
 * are the renderer's: `stream` first waits, on the device, for what the renderer has in flight -- look-ahead chunks included, none is
 * discarded -- and the renderer's next use of the buffers, on whatever stream, waits for the query. */
int tinsel_hip_trace_radiance_device(tinsel_hip* r, long long n, const tinsel_path_start* starts_dev, int max_depth, float* out_rgbx_dev, void* stream);

/* Gather queries on the resident scene: `samples` paths from each of n surface points, drawn and reduced on the device -- one mean
 * radiance per point for light-map baking, probe baking and radiance caches, where n*samples tinsel_path_start records in and as many
 * results out would be the whole cost.  A point is a position (the origin as given: the caller applies its own offset off the surface),
 * the shutter time, a normal (used as given: the caller supplies unit length) and a seed.
 * Sample s of point k (0 <= s < samples): the generator is the reference's Random(seed_k + s), the sum wrapping in 32 bits;
 * u1 = Randf(), then u2 = Randf().  TINSEL_GATHER_COSINE: BasisFromVector(n, &u, &v), d = CosineSampleHemisphere(u1, u2), direction
 * u*d.x + v*d.y + n*d.z -- the basis as render.cpp:328 builds it, the sum in the operand order of disney.h:256-258
 * (`U*d.x + V*d.y + N*d.z`, added left to right).  TINSEL_GATHER_SPHERE: direction UniformSampleSphere(u1, u2), the normal ignored.
 * PathTrace (render.cpp:230-388) is entered with that ray, the point's time and the generator as it stands after the two draws:
 * rng1 / rng2 of tinsel_path_start for Random(seed_k + s) advanced twice.  Callers who want independent streams space their seeds by
 * at least `samples`.
 * out[4*k .. 4*k + 2] is the sum over s = 0 .. samples - 1, in ascending s, in fp32, without contraction, of what PathTrace returns for
 * sample s, divided by (float)samples with an IEEE divide (TINSEL_ARITH_EXACT); out[4*k + 3] is reserved and written as 0.  Unclamped and
 * unfiltered, as for radiance queries.  COSINE: mean * pi is the irradiance, mean * albedo a Lambertian surface's exitant radiance;
 * SPHERE: the mean incident radiance (a light probe).
 * starts_out, when not NULL, receives the generated tinsel_path_start of path (k, s) at index k*samples + s, reserved words 0, whatever
 * order the device traced them in: tinsel_hip_trace_radiance on it gives the summands (re-tracing a firefly).
 * Everything else is as for radiance queries: the scene in force and the renderer's roulette, probe-sampling and arithmetic settings;
 * the shard ignored, no tinsel_hip_init needed; accumulator, pass index, pass seeds, tuning and look-ahead untouched; rays and samples
 * counted in tinsel_hip_stats; the paired pipeline where a render would run it and the split pipeline otherwise, behind kernel
 * "k_generate_gather" and in front of "k_gather_reduce" in tinsel_hip_kernel_times.  A batch holds whole points only,
 * floor(batch_paths / samples) of them (one at least); batches run one after the other and the result does not depend on the cut.
 * Bad arguments -- a null renderer, a mode out of range, n < 0 or n >= 2^31, samples outside [1, 65536], max_depth < 1, a null points or
 * out array with n > 0, a moved primitive without tinsel_hip_rebuild_scene -- return -1 and launch nothing; n == 0 returns 0.  The
 * arguments and the scene are judged before n is looked at: n == 0 with a mode out of range, or with a moved primitive, returns -1.
 * Memory: the path buffers of a batch as for radiance queries, plus 16 bytes per path of the batch kept until tinsel_hip_destroy (the
 * paths' radiance, which the reduction reads).  The host entry stages through the buffers of tinsel_hip_trace_rays /
 * tinsel_hip_trace_radiance, at most 64 MB whatever n and samples are: 2^20 points per chunk (32 MB of points, 16 MB of means); with
 * starts_out a chunk is min(2^20, floor(64 MB / (48 + 48*samples))) points, so that points, means and one chunk's records (in a third
 * buffer of the renderer's) stay below the same ceiling. */
typedef struct tinsel_gather_point { float px, py, pz, time;  float nx, ny, nz;  uint32_t seed; } tinsel_gather_point;

#define TINSEL_GATHER_COSINE 0   /* cosine-weighted hemisphere about the normal: mean * pi = irradiance, mean * albedo = Lambertian exitant radiance */
#define TINSEL_GATHER_SPHERE 1   /* uniform sphere, normal ignored: mean incident radiance (a light probe) */

/* host arrays (staged in chunks); returns when `out_rgbx_host` (and `starts_out_host`) is written */
int tinsel_hip_gather_radiance(tinsel_hip* r, int mode, long long n, const tinsel_gather_point* points_host, int samples, int max_depth,
                               float* out_rgbx_host, tinsel_path_start* starts_out_host /* may be NULL */);
/* device arrays, 16-byte aligned, not overlapping; enqueued on `stream` (NULL: the default stream) and not waited for, ordered against the
 * renderer's own work as tinsel_hip_trace_radiance_device is */
int tinsel_hip_gather_radiance_device(tinsel_hip* r, int mode, long long n, const tinsel_gather_point* points_dev, int samples, int max_depth,
                                      float* out_rgbx_dev, tinsel_path_start* starts_out_dev /* may be NULL */, void* stream);

/* SH gather queries: a gather query whose paths are projected onto the real spherical harmonics of bands 0 .. order instead of averaged
 * to one colour -- what a light probe keeps of its directions.  `order` is the highest band, 0, 1 or 2; C = (order + 1)^2 coefficients
 * per channel come back.  The point record, the modes, the seeds, the two draws, the directions, starts_out, the batch rule (whole points
 * only), the stream ordering, what is left untouched, the statistics and the bad-argument rules are those of tinsel_hip_gather_radiance*;
 * in addition an order outside 0 .. TINSEL_GATHER_SH_MAX_ORDER returns -1 (judged with the other arguments, before n is looked at).
 * out holds n*C float4: out[(k*C + i)*4 + c] is coefficient i, channel c (0, 1, 2 = r, g, b) of point k; word 3 of every float4 is
 * written as 0.  The value is the plain mean, no 4 pi or pi folded in:
 *     acc[i][c] = acc[i][c] + L[s][c] * Y_i(d_s)   for s = 0 .. samples - 1 in ascending order, then acc[i][c] / (float)samples
 * -- the product rounded to fp32, then the sum, no contraction, and an IEEE divide (TINSEL_ARITH_EXACT) -- where L[s] is what PathTrace
 * returns for sample s and d_s = (x, y, z) the direction the path was generated with: the bits of starts_out[k*samples + s].dx, dy, dz.
 * The basis is the real orthonormal one of the graphics convention, in fp32 and in this operation order:
 *     Y0 = 0.28209479f
 *     Y1 = 0.48860251f*y        Y2 = 0.48860251f*z        Y3 = 0.48860251f*x
 *     Y4 = (1.0925484f*x)*y     Y5 = (1.0925484f*y)*z     Y7 = (1.0925484f*x)*z
 *     Y6 = 0.31539157f*((3.0f*z)*z - 1.0f)
 *     Y8 = 0.54627422f*(x*x - y*y)
 * What the means are: TINSEL_GATHER_SPHERE draws with density 1/(4 pi), so 4 pi * mean_i are the SH coefficients of the incident radiance
 * (convolved with the cosine lobe -- factors pi, 2 pi/3, pi/4 for bands 0, 1, 2 -- they give the irradiance for any normal);
 * TINSEL_GATHER_COSINE draws with density cos/pi about the normal, so pi * mean_i are the coefficients of the cosine-weighted incident
 * radiance about that normal, and pi * mean_0 / Y0 is the irradiance.
 * Kernels: "k_generate_gather" in front, the pipeline, and "k_gather_sh_reduce" behind it ("k_gather_reduce" does not run); the reduction
 * derives every path's direction again from the point record and s, nothing is stored per path beyond the 16 bytes of radiance a gather
 * query keeps, in the same buffer.  The host entry stages as tinsel_hip_gather_radiance does, under the same 64 MB ceiling: a chunk is
 * min(2^20, floor(64 MB / (32 + 16*C [+ 48*samples with starts_out]))) points. */
#define TINSEL_GATHER_SH_MAX_ORDER 2

/* host arrays (staged in chunks); returns when `out_host` (and `starts_out_host`) is written */
int tinsel_hip_gather_sh(tinsel_hip* r, int mode, int order, long long n, const tinsel_gather_point* points_host,
                         int samples, int max_depth, float* out_host, tinsel_path_start* starts_out_host /* may be NULL */);
/* device arrays, 16-byte aligned, not overlapping; enqueued on `stream` (NULL: the default stream) and not waited for, ordered against the
 * renderer's own work as tinsel_hip_trace_radiance_device is */
int tinsel_hip_gather_sh_device(tinsel_hip* r, int mode, int order, long long n, const tinsel_gather_point* points_dev,
                                int samples, int max_depth, float* out_dev, tinsel_path_start* starts_out_dev /* may be NULL */, void* stream);

/* Allocates the per-batch path buffers a later render of `passes` passes at `max_depth` will need, so that the first
 * such call does not pay for hipMalloc (tinsel_hip_render* allocate on demand otherwise). */
int tinsel_hip_reserve(tinsel_hip* r, int passes, int max_depth);

/* Upper bound on path slots resident per batch (default 64 Mi for the wavefront pipelines, 8 Mi for the megakernel arm); the
 * same field as tinsel_hip_tuning::batch_paths. */
int tinsel_hip_set_batch_paths(tinsel_hip* r, unsigned long long max_paths);

/* Per-path radiance of the most recent batch (test hook): copies min(max_paths, paths in batch)
 * float4 records {r,g,b,-} in slot order (slot = pass_in_batch*W*H + j*W + i) and returns the count. */
long long tinsel_hip_read_batch_radiance(tinsel_hip* r, float* out_rgbx, unsigned long long max_paths);

/* Test hook: evaluates one device leaf function on caller arrays (host pointers; rows of `in_stride` /
 * `out_stride` floats, one thread per row) so tests can table the HIP restatements against the reference's
 * inline functions.  op: 0 Random, 1 CameraSampler::GenerateRay, 2 BSDFEval+BSDFPdf, 3 BSDFSample,
 * 4 PrimitiveIntersect, 5 PrimitiveSample, 6 ProbeSample/ProbePdf/Sky::Eval, 7 libm restatements,
 * 8 display-stage functions (row layouts: tn_kernels.h LeafOp).
 * `index` = primitive (its material for ops 2,3).
 * The hook follows the renderer's arithmetic arm: the exact build's functions by default, the tolerance build's (the same kernel
 * compiled from tinsel_fast.hip) after tinsel_hip_set_arithmetic(r, TINSEL_ARITH_FAST) -- what tests/test_gpu_fast_leaf.py tables
 * against a float64 statement of the same functions (tests/shade_f64.py).  Random (op 0) is integer arithmetic: the same bits in both. */
int tinsel_hip_leaf(tinsel_hip* r, int op, int index, int n, const float* in, int in_stride, const uint32_t* seeds,
                    float* out, int out_stride, const tinsel_camera* camera, int width, int height);

/* Test hook: the tree of mesh primitive `primitive` that is in force now (the reference's or a device-built one,
 * tinsel_hip_set_mesh_bvh), as the kernels read it: `capacity` >= numInternal 64-B Node64 records (tn_scene.h: both
 * children's boxes {min.xyz, max.xyz}, then the left and right child refs, leaf bit 31 | triangle index) into `out_nodes`
 * (may be NULL: meta only).  out_meta[7] = {root ref, numInternal, numTris, stackNeed, topCount, twoLeaves, inArena}.
 * An arena mesh's tree is read from the arena's copy in HBM.  Synchronises.  Returns numInternal, or -1. */
int tinsel_hip_mesh_tree(tinsel_hip* r, int primitive, void* out_nodes, int capacity, int* out_meta);

/* Introspection: LDS traversal-stack entries per lane chosen for this scene, NEE rays per bounce. */
int tinsel_hip_stack_entries(tinsel_hip* r);
int tinsel_hip_nee_per_path(tinsel_hip* r);
/* Primitives whose mesh BVH is walked by the dedicated k_walk kernel ahead of the scan kernels (large meshes in HBM,
 * split pipeline; tn_walk.h).  0: every mesh is walked inline, as IntersectRayMesh is called in the reference. */
int tinsel_hip_walked_prims(tinsel_hip* r);
/* Introspection: the Node64 records of each walked primitive's tree that k_walk's workgroups would stage into LDS under the tuning in
 * force (the first records of its breadth-first top, tinsel_hip_mesh_tree's topCount at most): what is left of a workgroup's LDS beside
 * the traversal stacks is handed out in primitive order, so a later primitive may get a part of its top, or none.
 * out_counts[k]: the k-th walked primitive (primitive order).  Returns their number (<= 7), or -1 (capacity too small). */
int tinsel_hip_walk_tops(tinsel_hip* r, int* out_counts, int capacity);
/* Queue lengths of the LAST batch of the wavefront pipelines: out[b] = paths alive at the start of bounce b (entries of the
 * extension queue; bounce 0: the paths generated, tile padding of a shard included), out[max_bounces + b] = paths with
 * shadow rays at bounce b (split pipeline; 0 otherwise).  Synchronises.
 * Returns the number of bounces written (<= max_bounces), or -1. */
int tinsel_hip_queue_counts(tinsel_hip* r, uint32_t* out, int max_bounces);
/* The fused kernel's last launch: out[0] = the instance's kind (0 general, 1 general with detail counters, 2 closed static scene,
 * 3 deferred mesh walks with pools / sharing / sorted queues), out[1] = the feature bits the
 * scene and the plan asked for (TINSEL_BOUNCE_*).  Returns 0, or -1 when the renderer has not launched k_bounce yet. */
int tinsel_hip_bounce_plan(tinsel_hip* r, uint32_t* out2);
/* The SCENE's share of those bits (media, probe, motion, mesh walk, sphere, transmission) from a scene description alone: no device, no
 * renderer.  What a renderer created from `scene` with the default tuning reports until a primitive is moved or a mesh tree rebuilt. */
unsigned int tinsel_hip_scene_features(const tinsel_scene_desc* scene);
/* The pairing RULE on a scene description (no device, no renderer): among the planes whose leaf of the scene BVH is an "infinite" box,
 * two whose eight coefficients are finite and whose normal components are each other's bitwise negation (or both zeros of any sign)
 * are a pair, greedily in primitive order, no plane twice.  Writes up to `capacity` pairs as (a, b) primitive indices, a < b, into
 * out_pairs[2*capacity] (NULL: count only) and returns the number of pairs; *out_singles (where given) is the number of such planes left
 * single.  Whether a renderer of the scene HAS a plane table, and pairs in it, is decided at create: no table with fewer than four
 * such planes and no mesh in HBM, or beyond the flat scan; no pairs with two or more mesh primitives that all ride in the arena, or
 * with tinsel_hip_tuning::plane_pairs = 0.  tinsel_hip_plane_table reports what a live renderer holds. */
int tinsel_hip_scene_plane_pairs(const tinsel_scene_desc* scene, int32_t* out_pairs, int capacity, int* out_singles);
/* The plane table of the scene level in force: out2[0] = opposing pairs, out2[1] = single planes (both 0 where the scene has no table).
 * Follows tinsel_hip_rebuild_scene, tinsel_hip_refit_mesh and tinsel_hip_tuning::plane_pairs. */
int tinsel_hip_plane_table(tinsel_hip* r, int* out2);
/* 1 where a path of `scene` carries the SLIM state in the fused kernel's compiled instances (kinds 2 and 3), else 0: no media, probe, motion,
 * mesh walk or transmission among the bits above, and every material's `subsurface` is +0.0f BY ITS BITS (-0.0f is not).  A scene that is
 * not slim runs the general kernel (kind 0) whatever its bits; the bits themselves do not know about subsurface.  No device, no renderer. */
int tinsel_hip_scene_slim(const tinsel_scene_desc* scene);
/* BAKED INSTANCES.  The fused kernel's closed instance (kind 2) compiled once more for ONE scene: the wave-uniform scene level -- the plane
 * table, the leaf boxes and primitive records the flat scan visits, the lights' records and constants -- stated as compile-time constants
 * in a generated header, so that the kernel fetches none of it and holds none of it in scalar registers.  Same float operations on the same
 * operands in the same order: results are bit-identical to the library's own instance.  The library generates the text and launches the
 * result; compiling is the caller's (tinsel_amd/build.py bake(): hipcc with the library's own flags, -DTN_BAKED_HEADER naming the text,
 * csrc/tinsel_baked.hip, device code only).
 *
 * tinsel_hip_bake_source: the header for the scene level IN FORCE (after any move, refit, rebuild or tuning change).  Writes up to
 * `capacity` bytes of text into out_text (NULL: none), the key -- the sha256 of the text, 64 hex digits and a NUL -- into out_key65 (where
 * given), and into *out_bakeable 1 where a camera render of this renderer is planned with the closed instance (exactly plan_batch's rule),
 * else 0, with the failing condition as tinsel_hip_last_error().  Returns the text's length in bytes, or -1.  No device work. */
long long tinsel_hip_bake_source(tinsel_hip* r, char* out_text, unsigned long long capacity, char* out_key65, int* out_bakeable);
/* The same from a scene description and a tuning (NULL: the defaults), with no device and no renderer: the text, key and answer a renderer
 * created from them on a gfx950 device reports until its scene level changes. */
long long tinsel_hip_bake_source_desc(const tinsel_scene_desc* scene, const tinsel_hip_tuning* tuning, char* out_text, unsigned long long capacity,
                                      char* out_key65, int* out_bakeable);
/* Installs the gfx950 code object `image` (`bytes` long) compiled from the text whose key is `key`: loads it, finds the kernel by its
 * mangled name, raises its dynamic-LDS limit like the library's own.  how: TINSEL_BAKE_COMPILED or TINSEL_BAKE_FROM_CACHE (reported by
 * tinsel_hip_bake_status).  image == NULL with how == TINSEL_BAKE_NO_COMPILER only records why nothing is installed.  From then on a
 * launch planned as kind 2 runs the installed function WHILE `key` equals the key of the scene level in force, the arithmetic arm is
 * TINSEL_ARITH_EXACT and the bake mode (tinsel_hip_set_bounce_bake) is not 0; otherwise the library's instance runs, as before.  A second install
 * replaces the first.  Returns 0, or -1 (the previous module, if any, stays). */
int tinsel_hip_install_baked(tinsel_hip* r, const void* image, unsigned long long bytes, const char* key, int how);
/* out3[0] = the state (below), out3[1..2] = the launches the installed function has served (low, high word); out_key65 (where given): the
 * installed module's key, or the empty string.  TINSEL_BAKE_OFF: the bake mode is 0; _NOT_BAKEABLE: the plan would not pick kind 2;
 * _NONE: bakeable, nothing installed; _NO_COMPILER: the caller found no compiler (or its compile failed); _COMPILED / _FROM_CACHE: an
 * installed module whose key is the live one; _LDS_REFUSED: such a module, but the runtime did not raise its dynamic-LDS limit and this scene's
 * launches ask for more than the default one, so it serves none; _STALE: an installed module compiled for another scene level (the library's instance runs). */
int tinsel_hip_bake_status(tinsel_hip* r, uint32_t* out3, char* out_key65);
/* The bake mode of a renderer: -1 auto (the default) | 0: an installed baked instance never serves a launch and a caller should bake none |
 * 1: wanted whatever the reservation's size.  The library compiles nothing itself: the mode says whether an installed instance may serve
 * a launch and tells the caller when to bake (tinsel_amd's Renderer.reserve(): with 1 always, with -1 at reservations of one default
 * batch, 64 Mi path slots, or more).  It is a setting of its own and not a field of tinsel_hip_tuning, whose layout stays as it is; the
 * Python binding carries it beside the struct as abi.Tuning's `bounce_bake`.  Set returns 0, or -1 (mode out of range); results are
 * bit-identical under every mode. */
int tinsel_hip_set_bounce_bake(tinsel_hip* r, int mode);
int tinsel_hip_get_bounce_bake(tinsel_hip* r);
enum { TINSEL_BAKE_OFF = 0, TINSEL_BAKE_NOT_BAKEABLE = 1, TINSEL_BAKE_NO_COMPILER = 2, TINSEL_BAKE_COMPILED = 3, TINSEL_BAKE_FROM_CACHE = 4,
       TINSEL_BAKE_STALE = 5, TINSEL_BAKE_NONE = 6, TINSEL_BAKE_LDS_REFUSED = 7 };
enum { TINSEL_BOUNCE_MEDIA = 1, TINSEL_BOUNCE_PROBE = 2, TINSEL_BOUNCE_MOTION = 4, TINSEL_BOUNCE_MESH_WALK = 8, TINSEL_BOUNCE_SPHERE = 16,
       TINSEL_BOUNCE_TRANSMISSION = 32, TINSEL_BOUNCE_POOLS = 64, TINSEL_BOUNCE_SHARE = 128, TINSEL_BOUNCE_SORT = 256, TINSEL_BOUNCE_ROULETTE = 512 };

const char* tinsel_hip_last_error(void);

/* ------------------------------------------------------------------------- */
/* All GPUs of one node behind ONE Renderer (tinsel_hip_create(scene, num_gpus); north_star: pixel   */
/* tiles sharded over the 8 GPUs with an RCCL reduce of the float4 accumulation buffer).                            */
/*                                                                                                                   */
/* The reference's caller is one single-threaded C++ loop (main.cpp:207 creates the renderer, :246-250 calls         */
/* Render): a group gives that caller N devices with no second process and no Python.  One host thread per device    */
/* drives a full tinsel_hip renderer of its own (scene uploaded to every device, rank-local path slots: set_shard);  */
/* every member traces the paths of ITS pixel tiles for every pass of a call, seeds depend on (pixel, pass) only, so  */
/* the sum over members of the accumulators is the single-GPU image up to float summation order.  That sum is ONE    */
/* ncclReduce(SUM, float, 4*W*H) over xGMI into a buffer on member 0 per read-back (the members' own accumulators    */
/* are never modified by it, so repeated calls cannot double-count), followed by the D2H copy.  RCCL is loaded with  */
/* dlopen on first use (librccl.so.1): a single-GPU user of this library needs no RCCL at all.                       */

typedef struct tinsel_hip_group tinsel_hip_group;      /* opaque */

/* Replaces `new GpuRenderer(scene)` for `num_gpus` devices (0 = every visible device), devices 0..num_gpus-1, pixel
 * tiles of `tile` x `tile` (0 = 64) dealt round-robin.  num_gpus == 1 is exactly one tinsel_hip (no RCCL, no threads'
 * worth of difference in the image).  Fails (NULL + tinsel_hip_last_error) when fewer devices are visible -- except
 * under TINSEL_HIP_GROUP_ONE_DEVICE=1, a VALIDATION switch for single-GPU boxes: all members share device 0 and the
 * reduce is a device-local sum in rank order instead of the RCCL call (threads, shards, slots and read-back as real). */
tinsel_hip_group* tinsel_hip_group_create(const tinsel_scene_desc* scene, int num_gpus, int tile);
/* The same with a tuning for every member (NULL: the defaults). */
tinsel_hip_group* tinsel_hip_group_create_tuned(const tinsel_scene_desc* scene, int num_gpus, int tile, const tinsel_hip_tuning* tuning);
void tinsel_hip_group_destroy(tinsel_hip_group* g);
/* Renderer::Init on every member (+ the reduce target on member 0). */
int tinsel_hip_group_init(tinsel_hip_group* g, int width, int height);
/* Renderer::Render: `passes` more samples per pixel of the WHOLE frame (each member its tiles), then -- when out_rgba
 * is not NULL -- reduce + copy the running sum of everything since Init to out_rgba (W*H*4 floats, host). */
int tinsel_hip_group_render(tinsel_hip_group* g, const tinsel_camera* camera, const tinsel_options* options, float* out_rgba, int passes);
/* Look-ahead for the reference's call pattern (tinsel_hip_set_lookahead) with N members: after a read-back every member
 * goes on with the calls that will most probably follow (same camera, options, pass count) -- a batch of up to 16 calls of
 * ITS shard traced at once, one snapshot accumulator per call -- and the NEXT call's snapshots are reduced (one
 * ncclReduce, each member from its own thread and stream) while this call's sum crosses PCIe.  A matching call waits
 * for that reduce (done, as a rule), swaps two buffers and copies; anything else drops the speculation.  Images are
 * those of the plain path bit for bit.  `enable` as for tinsel_hip_set_lookahead (a group of one forwards to it). */
int tinsel_hip_group_set_lookahead(tinsel_hip_group* g, int enable);
/* The display stage (tinsel_hip_present) on the reduced accumulator, run on member 0. */
int tinsel_hip_group_present(tinsel_hip_group* g, const tinsel_options* options, int nlm_width, float nlm_falloff, float* out_rgba);
int tinsel_hip_group_size(tinsel_hip_group* g);
/* Member `rank`'s renderer, for the introspection / statistics entry points (do not render or init through it).
 * Whatever the group had speculated is dropped first (look-ahead starts over with the next read-back). */
tinsel_hip* tinsel_hip_group_member(tinsel_hip_group* g, int rank);

/* One process per GPU (an MPI-style host: bench.py --gpus N under torch.distributed.run): the SAME collective as the group's -- one
 * ncclReduce(SUM, float, 4*W*H) of the accumulators to `root` -- with the communicator made by ncclCommInitRank.  The host language only
 * carries the 128-byte id from rank 0 to the other ranks (a torch.distributed broadcast, MPI_Bcast, a file); set_shard(rank, world, tile)
 * is the caller's, as before.  comm_init is collective (every rank calls it); comm_size = ncclCommCount of the communicator (0: none);
 * comm_reduce_accum enqueues on `stream`, WAITS for it, and leaves the sum in `out_device` (W*H*4 floats of device memory) on `root`
 * only -- this rank's own accumulator is never written, so a later render + reduce cannot count a sample twice. */
#define TINSEL_HIP_COMM_ID_BYTES 128
int tinsel_hip_comm_unique_id(unsigned char* id_bytes, int capacity);
int tinsel_hip_comm_init(tinsel_hip* r, const unsigned char* id_bytes, int rank, int world);
int tinsel_hip_comm_size(tinsel_hip* r);
int tinsel_hip_comm_reduce_accum(tinsel_hip* r, float* out_device, int root, void* stream);

/* How a batch of `slots` path slots is cut into regions on a device of `num_cus` CUs (the dense path state of the wavefront pipelines:
 * DESIGN.md section 4; `fused` != 0: the fused pipeline, which ends a batch with shorter regions).  Pure host arithmetic -- no device is
 * touched: out[6] = number of regions, positions per region, regions of that length (the rest are short), positions per short region,
 * workgroups of a launch, capacity of the region arrays.  Introspection for the tests; no reference counterpart. */
int tinsel_hip_plan_regions(unsigned long long slots, int num_cus, int nee_per_path, int fused, unsigned int* out);

/* Exhaustive self-test of the parity arm's short reciprocal / square-root sequences (tn_math.h rcp_candidate / sqrt_candidate):
 * compares the candidate with the compiler's correctly rounded `1.0f/x` (op 0), `sqrtf(x)` (op 1) or `1.0f/sqrtf(x)` (op 2) on ALL 2^32 fp32 bit patterns
 * on the device.  variant < 0: the variant this library's kernels are built with (0 = the compiler's own expansion).
 * out_counts[260]: [0..3] mismatches in total / with a denormal operand / with |x| >= 2^126 (op 0) or x < 0 (ops 1, 2) / any
 * other; [4 + e] mismatches by the operand's exponent field e;
 * out_first_bad: the smallest mismatching bit pattern (0xffffffff when none).  No reference counterpart (test infrastructure
 * of this library: the reference divides with the host FPU / nvcc's IEEE division, render.cpp / maths.h throughout). */
int tinsel_hip_selftest_arith(int device_index, int op, int variant, unsigned long long* out_counts, unsigned int* out_first_bad);
/* The library's own stable radix sort and exclusive scan (the device BVH builder's, tinsel_amd/csrc/tn_sort.h) on caller data, for tests:
 * keys[0, n) sorted in place by their bits [begin_bit, end_bit) (multiples of 8; keys with equal bits keep their order);
 * out[i] = in[0] + .. + in[i - 1]. */
int tinsel_hip_selftest_sort(int device_index, unsigned long long* keys, unsigned long long n, int begin_bit, int end_bit);
int tinsel_hip_selftest_scan(int device_index, const int* in, int* out, unsigned long long n);
/* Does the accumulate stage take its support form for this filter (1) or not (0)?  The form gathers, per pixel, only the samples generated at the
 * pixel and its upper / left neighbours: a Gaussian filter of width <= 1 with offset > 0 whose weight max(0, expf(a) - offset) is +0 by
 * construction from one pixel away on -- a = -falloff*x*x <= *out_arg_zero = log(offset) - 1e-6 (double, rounded down to float) for |x| >= 1.
 * Host arithmetic only; out_arg_zero may be NULL. */
int tinsel_hip_accumulate_support(int filter_type, float filter_width, float filter_falloff, float filter_offset, float* out_arg_zero);
/* The accumulate stage (the reference's CpuRenderer::AddSample, render.cpp:401-445, over whole passes) on caller data, for tests: the paths of pass s
 * generated at pixel (i, j) have the raster position Random(i + j*width + pass_seeds[s]) draws and the radiance radiance[(s*height + j)*width + i]
 * (rgbx); they are added to accum[height*width] (rgba, in/out) by exactly the launch a render of such a frame makes on this device (one shard).
 * choice: tinsel_hip_tuning::accumulate.  form 0: as the library decides | 1: the full candidate window | 2: the support form (Gaussian filters
 * whose weight is +0 by construction a pixel away from the sample; an error where the filter or the chosen kernel has no such form).
 * *out_form: what ran -- 0 k_accumulate | 1 k_accumulate_tiled, 256 threads | 2 the same, 512 | 3 k_accumulate_piped | 4 / 5 the support form of 1 / 2. */
int tinsel_hip_selftest_accumulate(int device_index, int width, int height, int filter_type, float filter_width, float filter_falloff, float filter_offset,
                                   float clamp, const unsigned int* pass_seeds, int passes, const float* radiance, float* accum, int choice, int form,
                                   int* out_form);

/* Yard-sticks measured on the GPU itself, for bench.py's roofline (not part of the render path): kind 0 = a float4 stream
 * copy of `bytes` bytes (*out_units = bytes read + written); kinds 1..3 = dependent chases through a table of 64-B records
 * of `bytes` bytes (rounded down to a power of two), `steps` visits per lane, 16 waves per CU (*out_units = records
 * visited) -- the access pattern of a BVH walk; the kind only names the kernel for the profiler: 1 a table beyond the
 * Infinity Cache (calibrates FETCH_SIZE for random 64-B gathers), 2 one the size of a walked tree, 3 one inside an L2.
 * *out_ms = the timed launch (HIP events). */
int tinsel_hip_ubench(int device_index, int kind, unsigned long long bytes, int steps, double* out_ms, double* out_units);

/* ------------------------------------------------------------------------- */
/* Scene packs: a relocatable single-blob serialisation of tinsel_scene_desc   */
/* (+ the scene's camera/options) so that scenes travel to machines without    */
/* the reference's loader.  See DESIGN.md "Scene pack".                         */

#define TINSEL_PACK_MAGIC "TINPACK1"

typedef struct tinsel_pack_header {
    char magic[8];
    uint32_t version;               /* 1 */
    uint32_t num_primitives;
    uint32_t num_bvh_nodes;
    uint32_t num_meshes;
    uint64_t total_bytes;
    uint64_t off_primitives;        /* tinsel_primitive[]; mesh pointer fields hold BYTE OFFSETS into the blob */
    uint64_t off_bvh_nodes;
    uint64_t off_probe_data;        /* 0 when there is no probe */
    uint64_t off_probe_pdf_x;
    uint64_t off_probe_cdf_x;
    uint64_t off_probe_pdf_y;
    uint64_t off_probe_cdf_y;
    int32_t probe_width;
    int32_t probe_height;
    tinsel_vec3 sky_horizon;
    tinsel_vec3 sky_zenith;
    tinsel_camera camera;
    tinsel_options options;
    uint8_t _reserved[48];
} tinsel_pack_header;

/* Resolves the offsets of a pack blob (in place: `blob` must stay alive and
 * writable) into a tinsel_scene_desc whose pointers point into the blob. */
int tinsel_pack_open(void* blob, size_t size, tinsel_scene_desc* out_scene,
                     tinsel_camera* out_camera, tinsel_options* out_options);

#ifdef __cplusplus
}

static_assert(sizeof(tinsel_vec3) == 12, "Vec3");
static_assert(sizeof(tinsel_transform) == 32, "Transform");
static_assert(sizeof(tinsel_bvh_node) == 32, "BVHNode");
static_assert(sizeof(tinsel_camera) == 40, "Camera");
static_assert(sizeof(tinsel_texture) == 24, "Texture");
static_assert(sizeof(tinsel_material) == 128, "Material");
static_assert(offsetof(tinsel_material, eta) == 36, "Material.eta");
static_assert(offsetof(tinsel_material, transmission) == 80, "Material.transmission");
static_assert(offsetof(tinsel_material, bump_map) == 88, "Material.bumpMap");
static_assert(offsetof(tinsel_material, bump) == 112, "Material.bump");
static_assert(sizeof(tinsel_mesh_geometry) == 64, "MeshGeometry");
static_assert(offsetof(tinsel_mesh_geometry, num_vertices) == 40, "MeshGeometry.numVertices");
static_assert(offsetof(tinsel_mesh_geometry, area) == 52, "MeshGeometry.area");
static_assert(offsetof(tinsel_mesh_geometry, id) == 56, "MeshGeometry.id");
static_assert(sizeof(tinsel_primitive) == 272, "Primitive");
static_assert(offsetof(tinsel_primitive, type) == 64, "Primitive.type");
static_assert(offsetof(tinsel_primitive, geo) == 72, "Primitive.geo");
static_assert(offsetof(tinsel_primitive, material) == 136, "Primitive.material");
static_assert(offsetof(tinsel_primitive, light_samples) == 264, "Primitive.lightSamples");
static_assert(sizeof(tinsel_filter) == 16, "Filter");
static_assert(sizeof(tinsel_options) == 48, "Options");
static_assert(offsetof(tinsel_options, max_depth) == 40, "Options.maxDepth");
static_assert(sizeof(tinsel_pack_header) == 256, "pack header");
static_assert(sizeof(tinsel_hip_tuning) == 128, "tuning");
static_assert(sizeof(tinsel_ray) == 32, "ray");
static_assert(sizeof(tinsel_ray_hit) == 32, "ray hit");
static_assert(sizeof(tinsel_path_start) == 48, "path start");
static_assert(sizeof(tinsel_gather_point) == 32, "gather point");
#endif

#endif /* TINSEL_HIP_H */

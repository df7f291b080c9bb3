// tn_launch.h -- the launches of the path kernels, as one function of a plain argument block.
//
// The library carries the path kernels TWICE, from two translation units built with different floating-point contracts:
//   tinsel_hip.hip   (namespace tn)        -ffp-contract=off, IEEE divide / sqrt, glibc's transcendentals restated:
//                                          bit-identical to the CPU oracle -- the default and the parity path;
//   tinsel_fast.hip  (namespace tn_fast)   FMA contraction, v_rcp / v_rsq / v_sqrt, hardware sin / cos / exp:
//                                          the opt-in tolerance arm (tinsel_hip_set_arithmetic), like the reference's
//                                          own `-O3 -ffast-math` / `-use_fast_math` builds (makefile:4, tinsel.vcxproj:134).
// Both include this header (the second one with `tn` renamed), so the two arms differ in arithmetic only: same kernels,
// same queues, same launch geometry.  The host plans the instance of every launch (plan_batch), fills a LaunchArgs per launch
// and hands it to launch_path_kernel of the arm in force, which launches entry `variant` of the list below.
#pragma once

#include "tn_kernels.h"

namespace tn {

// Every path-kernel instance the host launches: id, workgroup, 1 where create raises its dynamic-LDS limit, arguments, instance (in code-object
// order).  COUNT: detail counters; FIT: k_bounce compiled for a fixed feature set (tn_fused.h); LDS: the whole scene in LDS; MIXED: the arena staged, meshes in HBM; W1 / W2: walked_only_level.
#define TN_PATH_KERNELS(X)                                                                                          \
    X(PK_GENERATE,              kBlock, 0, GENERATE, k_generate)                                                    \
    X(PK_EXTEND_W2_MIXED,       kBlock, 0, EXTEND,   k_extend<false, true, 2, true>)                                \
    X(PK_EXTEND_W1_MIXED,       kBlock, 0, EXTEND,   k_extend<false, true, 1, true>)                                \
    X(PK_EXTEND_W1,             kBlock, 0, EXTEND,   k_extend<false, false, 1>)                                     \
    X(PK_EXTEND_MIXED_LIGHTS,   kBlock, 0, EXTEND,   k_extend<false, true, 0, true, true>)                          \
    X(PK_EXTEND_MIXED,          kBlock, 0, EXTEND,   k_extend<false, true, 0, true>)                                \
    X(PK_EXTEND_COUNT_LDS,      kBlock, 0, EXTEND,   k_extend<true, true>)                                          \
    X(PK_EXTEND_COUNT,          kBlock, 0, EXTEND,   k_extend<true, false>)                                         \
    X(PK_EXTEND_LDS,            kBlock, 0, EXTEND,   k_extend<false, true>)                                         \
    X(PK_EXTEND,                kBlock, 0, EXTEND,   k_extend<false, false>)                                        \
    X(PK_SHADOW_W2_MIXED,       kBlock, 0, SHADOW,   k_shadow<false, true, 2, true>)                                \
    X(PK_SHADOW_W1_MIXED,       kBlock, 0, SHADOW,   k_shadow<false, true, 1, true>)                                \
    X(PK_SHADOW_W1,             kBlock, 0, SHADOW,   k_shadow<false, false, 1>)                                     \
    X(PK_SHADOW_MIXED,          kBlock, 0, SHADOW,   k_shadow<false, true, 0, true>)                                \
    X(PK_SHADOW_COUNT_LDS,      kBlock, 0, SHADOW,   k_shadow<true, true>)                                          \
    X(PK_SHADOW_COUNT,          kBlock, 0, SHADOW,   k_shadow<true, false>)                                         \
    X(PK_SHADOW_LDS,            kBlock, 0, SHADOW,   k_shadow<false, true>)                                         \
    X(PK_SHADOW,                kBlock, 0, SHADOW,   k_shadow<false, false>)                                        \
    X(PK_MEGA_COUNT_LDS,        kBlock, 0, MEGA,     k_mega<true, true>)                                            \
    X(PK_MEGA_COUNT,            kBlock, 0, MEGA,     k_mega<true, false>)                                           \
    X(PK_MEGA_LDS,              kBlock, 0, MEGA,     k_mega<false, true>)                                           \
    X(PK_MEGA,                  kBlock, 0, MEGA,     k_mega<false, false>)                                          \
    X(PK_COST_LDS,              kBlock, 0, COST,     k_cost<true>)                                                  \
    X(PK_COST,                  kBlock, 0, COST,     k_cost<false>)                                                 \
    X(PK_LIGHTS_MIXED,          kBlock, 0, LIGHTS,   k_lights<true, true>)                                          \
    X(PK_LIGHTS_LDS,            kBlock, 0, LIGHTS,   k_lights<true>)                                                \
    X(PK_LIGHTS,                kBlock, 0, LIGHTS,   k_lights<false>)                                               \
    X(PK_SHADE_SORTED_MIXED,    kBlock, 1, SHADE,    k_shade_sorted<true, true>)                                    \
    X(PK_SHADE_SORTED_LDS,      kBlock, 1, SHADE,    k_shade_sorted<true>)                                          \
    X(PK_SHADE_SORTED,          kBlock, 1, SHADE,    k_shade_sorted<false>)                                         \
    X(PK_SHADE_MIXED,           kBlock, 0, SHADE,    k_shade<true, true>)                                           \
    X(PK_SHADE_LDS,             kBlock, 0, SHADE,    k_shade<true>)                                                 \
    X(PK_SHADE,                 kBlock, 0, SHADE,    k_shade<false>)                                                \
    X(PK_BOUNCE_COUNT_LDS,      kBlock, 1, BOUNCE,   k_bounce<kBounceCount, true, false>)                           \
    X(PK_BOUNCE_COUNT,          kBlock, 1, BOUNCE,   k_bounce<kBounceCount, false, false>)                          \
    X(PK_BOUNCE_LDS_DEFER,      kBlock, 1, BOUNCE,   k_bounce<kBounceGeneral, true, true>)                          \
    X(PK_BOUNCE_DEFER,          kBlock, 1, BOUNCE,   k_bounce<kBounceGeneral, false, true>)                         \
    X(PK_BOUNCE_LDS,            kBlock, 1, BOUNCE,   k_bounce<kBounceGeneral, true, false>)                         \
    X(PK_BOUNCE,                kBlock, 1, BOUNCE,   k_bounce<kBounceGeneral, false, false>)                        \
    X(PK_BOUNCE_FIT_CLOSED,     kBlock, 1, BOUNCE,   k_bounce<kBounceFitClosed, true, false>)                       \
    X(PK_BOUNCE_FIT_DEFERRED,   kBlock, 1, BOUNCE,   k_bounce<kBounceFitDeferred, true, true>)                      \
    X(PK_STEP_W2_MIXED,         kBlock, 0, STEP,     k_step<true, 2, true>)                                         \
    X(PK_STEP_W1_MIXED,         kBlock, 0, STEP,     k_step<true, 1, true>)                                         \
    X(PK_STEP_W1,               kBlock, 0, STEP,     k_step<false, 1, false>)                                       \
    X(PK_STEP_MIXED,            kBlock, 0, STEP,     k_step<true, 0, true>)                                         \
    X(PK_STEP_LDS,              kBlock, 0, STEP,     k_step<true, 0, false>)                                        \
    X(PK_STEP,                  kBlock, 0, STEP,     k_step<false, 0, false>)                                       \
    X(PK_SWALK_SHADOW_LDS,      1024,   1, SWALK,    k_swalk<true, 1024, 1>)                                        \
    X(PK_SWALK_SHADOW_MIXED,    1024,   1, SWALK,    k_swalk<true, 1024, 2>)                                        \
    X(PK_SWALK_SHADOW,          kBlock, 1, SWALK,    k_swalk<true, 256, 0>)                                         \
    X(PK_SWALK_EXTEND_LDS,      1024,   1, SWALK,    k_swalk<false, 1024, 1>)                                       \
    X(PK_SWALK_EXTEND_MIXED,    1024,   1, SWALK,    k_swalk<false, 1024, 2>)                                       \
    X(PK_SWALK_EXTEND,          kBlock, 1, SWALK,    k_swalk<false, 256, 0>)                                        \
    X(PK_WALK_SINGLE_1024X2,    1024,   1, WALK,     k_walk<1024, 8>)                                               \
    X(PK_WALK_SINGLE_1024,      1024,   1, WALK,     k_walk<1024, 4>)                                               \
    X(PK_WALK_SINGLE_256,       256,    1, WALK,     k_walk<256, 5>)                                                \
    X(PK_WALK_RAYS_1024X2,      1024,   1, WALK,     k_walk_rays<1024, 8>)                                          \
    X(PK_WALK_RAYS_1024,        1024,   1, WALK,     k_walk_rays<1024, 4>)                                          \
    X(PK_WALK_RAYS_256,         256,    1, WALK,     k_walk_rays<256, 5>)                                           \
    X(PK_QUERY_CLOSEST_LDS,     kBlock, 0, QUERY,    k_query<kQueryClosest, true>)                                  \
    X(PK_QUERY_CLOSEST,         kBlock, 0, QUERY,    k_query<kQueryClosest, false>)                                 \
    X(PK_QUERY_OCCLUDED_LDS,    kBlock, 0, QUERY,    k_query<kQueryOccluded, true>)                                 \
    X(PK_QUERY_OCCLUDED,        kBlock, 0, QUERY,    k_query<kQueryOccluded, false>)                                \
    X(PK_QUERY_CAMERA_LDS,      kBlock, 0, QUERY,    k_query<kQueryCamera, true>)                                   \
    X(PK_QUERY_CAMERA,          kBlock, 0, QUERY,    k_query<kQueryCamera, false>)                                  \
    X(PK_QUERYR_CLOSEST_LDS,    kBlock, 0, QUERY,    k_query_refill<kQueryClosest, true>)                           \
    X(PK_QUERYR_CLOSEST,        kBlock, 0, QUERY,    k_query_refill<kQueryClosest, false>)                          \
    X(PK_QUERYR_OCCLUDED_LDS,   kBlock, 0, QUERY,    k_query_refill<kQueryOccluded, true>)                          \
    X(PK_QUERYR_OCCLUDED,       kBlock, 0, QUERY,    k_query_refill<kQueryOccluded, false>)                         \
    X(PK_GENERATE_RAYS,         kBlock, 0, GENERATE_RAYS, k_generate_rays)                                          \
    X(PK_GENERATE_GATHER,       kBlock, 0, GENERATE_GATHER, k_generate_gather)                                      \
    X(PK_GATHER_REDUCE,         kBlock, 0, GATHER_REDUCE, k_gather_reduce)                                          \
    X(PK_GATHER_SH_REDUCE,      kShWave, 0, GATHER_SH_REDUCE, k_gather_sh_reduce)                                   \
    X(PK_FEATURES_LDS,          kBlock, 0, FEATURES, k_features<true>)                                              \
    X(PK_FEATURES,              kBlock, 0, FEATURES, k_features<false>)                                             \
    X(PK_IDS_LDS,               kBlock, 0, FEATURES, k_ids<true>)                                                   \
    X(PK_IDS,                   kBlock, 0, FEATURES, k_ids<false>)                                                  \
    X(PK_SHADE_GROUPS_MIXED,    kBlock, 0, SHADE_GROUPS, k_shade_groups<true, true>)                                \
    X(PK_SHADE_GROUPS_LDS,      kBlock, 0, SHADE_GROUPS, k_shade_groups<true>)                                      \
    X(PK_SHADE_GROUPS,          kBlock, 0, SHADE_GROUPS, k_shade_groups<false>)                                     \
    X(PK_GENERATE_VIEWS,        kBlock, 0, GENERATE_VIEWS, k_generate_views)                                        \
    X(PK_GENERATE_SAMPLES,      kBlock, 0, GENERATE_SAMPLES, k_generate_samples)                                    \
    X(PK_SHADE_DEPTHS_MIXED,    kBlock, 0, SHADE_DEPTHS, k_shade_depths<true, true>)                                \
    X(PK_SHADE_DEPTHS_LDS,      kBlock, 0, SHADE_DEPTHS, k_shade_depths<true>)                                      \
    X(PK_SHADE_DEPTHS,          kBlock, 0, SHADE_DEPTHS, k_shade_depths<false>)

enum PathKernel : int
{
    PK_NONE = 0,                    // not launched (and what a zeroed LaunchArgs names: no instance)
#define TN_ID(ID, BLOCK, PREP, ARGS, ...) ID,
    TN_PATH_KERNELS(TN_ID)
#undef TN_ID
};

struct LaunchArgs
{
    DevScene scene;                 // (scene.arenaLdsBytes: the arena bytes the launched kernel stages)
    PathState ps;
    SplitState ss;                  // the wavefront pipelines' dense state
    QueueCtl ctl;
    CameraParams cam;
    FrameParams fp;
    const uint32_t* passSeeds;
    const float4* walkRec;          // k_walk's records (null: meshes are walked inline)
    uint32_t walkPrims;
    const uint32_t* order;          // region groups, longest first (k_region_order; null: in index order)
    BinPrims bins;                  // primitives whose leaf-box test sorts the queues
    WalkJob walk;                   // k_walk
    SwalkJob swalk;                 // k_swalk
    int variant;                    // the instance launched (PathKernel)
    int bounce;
    int bounceEnd;                  // k_bounce: the launch covers the bounces [bounce, bounceEnd)
    int stackEntries;
    int grid;
    uint32_t ldsBytes;              // dynamic LDS of the launch
    uint32_t* cost;                 // k_cost: the cost map's four planes
    QueryJob query;                 // k_query
    RadianceJob radiance;           // k_generate_rays
    GatherJob gather;               // k_generate_gather, k_gather_reduce, k_gather_sh_reduce
    int shOrder;                    // k_gather_sh_reduce: the highest band
    FeatureJob features;            // k_features, k_ids
    GroupState groups;              // k_shade_groups
    ViewsJob views;                 // k_generate_views
    SamplesJob samples;             // k_generate_samples
    DepthState depths;              // k_shade_depths
};

#define TN_ARGS_GENERATE a.ss, a.ctl, a.cam, a.fp, a.passSeeds, a.scene.primBoxes, a.bins
#define TN_ARGS_EXTEND   a.scene, a.ss, a.ctl, a.bounce, a.stackEntries, a.walkRec, a.walkPrims, a.bins, a.order
#define TN_ARGS_SHADOW   a.scene, a.ss, a.ctl, a.bounce, a.stackEntries, a.walkRec, a.walkPrims, a.order
#define TN_ARGS_MEGA     a.scene, a.ps, a.ctl, a.cam, a.fp, a.passSeeds, a.stackEntries
#define TN_ARGS_COST     a.scene, a.cam, a.fp, a.passSeeds, a.stackEntries, a.cost
#define TN_ARGS_LIGHTS   a.scene, a.ss, a.bounce, a.bins, a.order
#define TN_ARGS_SHADE    a.scene, a.ss, a.bounce, a.fp.maxDepth, a.fp.rrStart, a.bins, a.order
#define TN_ARGS_BOUNCE   BounceKernargs{ a.scene, a.ss, a.ctl, a.bounce, a.bounceEnd, a.stackEntries, a.cam, a.fp, a.passSeeds }
#define TN_ARGS_STEP     a.scene, a.ss, a.ctl, a.bounce, a.fp.maxDepth, a.fp.rrStart, a.stackEntries, a.walkRec, a.walkPrims, a.bins, a.order
#define TN_ARGS_SWALK    a.scene, a.ss, a.ctl, a.bounce, a.swalk
#define TN_ARGS_WALK     a.scene, a.walk
#define TN_ARGS_QUERY    a.scene, a.query, a.cam, a.stackEntries
#define TN_ARGS_GENERATE_RAYS a.ss, a.ctl, a.radiance, a.scene.primBoxes, a.bins
#define TN_ARGS_GENERATE_GATHER a.ss, a.ctl, a.gather, a.scene.primBoxes, a.bins
#define TN_ARGS_GATHER_REDUCE a.ps.rad, a.gather
#define TN_ARGS_GATHER_SH_REDUCE a.ps.rad, a.gather, a.shOrder
#define TN_ARGS_FEATURES a.scene, a.features, a.cam, a.fp, a.passSeeds, a.stackEntries
#define TN_ARGS_SHADE_GROUPS TN_ARGS_SHADE, a.groups
#define TN_ARGS_GENERATE_VIEWS a.ss, a.ctl, a.views, a.fp, a.passSeeds, a.scene.primBoxes, a.bins
#define TN_ARGS_SHADE_DEPTHS TN_ARGS_SHADE, a.depths
#define TN_ARGS_GENERATE_SAMPLES a.ss, a.ctl, a.samples, a.cam, a.fp, a.passSeeds, a.scene.primBoxes, a.bins

// false: a.variant is not in the list (nothing is launched)
inline bool launch_path_kernel(const LaunchArgs& a, hipStream_t st)
{
    switch (a.variant)
    {
#define TN_LAUNCH(ID, BLOCK, PREP, ARGS, ...)                                                                          \
    case ID: hipLaunchKernelGGL((__VA_ARGS__), dim3((unsigned)a.grid), dim3(BLOCK), a.ldsBytes, st, TN_ARGS_##ARGS); return true;
        TN_PATH_KERNELS(TN_LAUNCH)
#undef TN_LAUNCH
    default:
        return false;
    }
}

// The entries marked 1 above (k_walk's tree tops, k_swalk, k_shade_sorted, k_bounce's pools beside a staged arena) ask for more dynamic LDS than
// the default launch limit: raised ONCE, at create, every result checked -- a device that grants less fails there with the kernel's name.
struct PrepReport
{
    int refused = 0;                // attributes the runtime refused
    const char* first = nullptr;    // the first kernel it refused
    int segPrefixLds = 0;           // the dynamic LDS k_seg_prefix may ask for (one count per region: the host clamps its grids to that)
};

inline void prep_lds(const void* kernel, const char* name, int bytes, PrepReport& rep)
{
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess)
    {
        (void)hipGetLastError();        // (a refused attribute must not surface as the next launch's error)
        if (!rep.first)
            rep.first = name;
        ++rep.refused;
    }
}

inline PrepReport prepare_path_kernels(int sharedMemLimit)
{
    PrepReport rep;
    // (k_seg_prefix has static LDS too)
    {
        PrepReport seg;
        prep_lds((const void*)k_seg_prefix, "k_seg_prefix", sharedMemLimit - 1024, seg);
        rep.segPrefixLds = seg.refused ? (sharedMemLimit < 65536 ? sharedMemLimit : 65536) - 1024 : sharedMemLimit - 1024;
        if (seg.refused) { rep.refused += 1; rep.first = rep.first ? rep.first : "k_seg_prefix"; }
    }
#define TN_PREP(ID, BLOCK, PREP, ARGS, ...) if (PREP) prep_lds((const void*)__VA_ARGS__, #__VA_ARGS__, sharedMemLimit, rep);
    TN_PATH_KERNELS(TN_PREP)
#undef TN_PREP
    return rep;
}

} // namespace tn

// tinsel_hip.hip -- host side of the C-ABI (include/tinsel_hip.h): scene flattening/upload,
// camera set-up, batch scheduling of the streaming pipeline, statistics and timing.
//
// Replaces the reference's GpuRenderer (src/render.cu:978-1110).  Built only with
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off  (tinsel_amd/build.py)

#include "../../include/tinsel_hip.h"

#include "tn_launch.h"
#include "tn_denoise.h"         // (this translation unit only: the denoise stage has no tolerance arm)
#include "tn_lbvh.h"
#include "tn_ubench.h"
#include "tn_selftest.h"

#include "tn_sort.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>          // types only: the library is dlopen'ed by the first multi-GPU group (no link-time dependency)

#include <dlfcn.h>

#include <cmath>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

using namespace tn;

namespace {

thread_local std::string g_error;

int fail(const std::string& msg)
{
    g_error = msg;
    fprintf(stderr, "tinsel_hip: %s\n", msg.c_str());
    return -1;
}

#define HIP_TRY(expr)                                                                                       \
    do {                                                                                                    \
        hipError_t _e = (expr);                                                                             \
        if (_e != hipSuccess)                                                                               \
            return fail(std::string(#expr) + ": " + hipGetErrorString(_e));                                 \
    } while (0)

#define HIP_TRY_NULL(expr)                                                                                  \
    do {                                                                                                    \
        hipError_t _e = (expr);                                                                             \
        if (_e != hipSuccess) {                                                                             \
            fail(std::string(#expr) + ": " + hipGetErrorString(_e));                                        \
            return nullptr;                                                                                 \
        }                                                                                                   \
    } while (0)

} // namespace

// The host side by concern, one translation unit (the kernels and everything above are shared):
#include "tn_host_own.h"          // DevBuf, DevPool, Stream, Event, PinnedOutput: the only file that allocates or frees
#include "tn_host_layout.h"       // BVH re-layout, arena
#include "tn_host_state.h"        // struct tinsel_hip
#include "tn_host_bake.h"         // baked instances: the generated scene-level header, its key, the installed module's launch
#include "tn_host_batch.h"        // launches, grids and regions, render_batch / render_impl
#include "tn_host_query.h"        // ray queries: k_query's plan and launch, the host entries' staging buffers
#include "tn_host_radiance.h"     // radiance queries: the split / paired pipeline on paths the caller starts
#include "tn_host_gather.h"       // gather queries: many paths per surface point, drawn and reduced on the device
#include "tn_host_features.h"     // feature buffers: albedo, normal and depth of the camera's own paths through the accumulate stage
#include "tn_host_ids.h"          // ID mattes: the hit primitive of the camera's own paths, gathered into ranked per-pixel (id, weight) lists
#include "tn_host_light_groups.h" // light groups: the beauty split per emitter group, k_shade_groups behind a render's split plan
#include "tn_host_views.h"        // view batches: many cameras' frames in one call, k_generate_views in front of a query's pipeline, k_views_accumulate behind it
#include "tn_host_depth_planes.h" // depth planes: the beauty at several path depths in one trace, k_shade_depths behind a render's split plan, k_views_accumulate behind it
#include "tn_host_samples.h"     // sample maps: a per-pixel pass count on compact slots, k_generate_samples in front of a query's pipeline, k_samples_accumulate behind it
#include "tn_host_denoise.h"      // the feature-guided denoise stage on linear radiance
#include "tn_host_lookahead.h"    // the one-pass-per-call pattern
#include "tn_host_bvh_build.h"    // device BVH build
#include "tn_host_scene.h"        // the scene level: derived and uploaded in one place; set_mesh_bvh / refit / move / rebuild_scene

// ===========================================================================
// C-ABI
#include "tn_host_create.h"       // create / destroy
#include "tn_host_api.h"          // everything else of include/tinsel_hip.h for one device
#include "tn_host_group.h"        // tinsel_hip_group

// tn_host_batch.h -- one batch of passes: timers, kernel launches, grids and regions, render_batch / render_impl
// (part of the library's one host translation unit: included by tinsel_hip.hip, in this order, never on its own)
#pragma once

namespace {

void free_batch(tinsel_hip* r)
{
    r->batchMem.release();
    for (tinsel_hip::DenseLane& lane : r->lane)
        lane = tinsel_hip::DenseLane();
    r->batchPipeline = -1;
    r->batchSlots = 0;
    r->batchStateSlots = 0;
    r->batchLanes = 1;
    r->batchNee = -1;
    r->batchDepth = -1;
    r->lastBatchSlots = 0;          // (tinsel_hip_read_batch_radiance: the batch's radiance went with the buffers)
}

// blocks per CU of the streaming kernels' fixed grid.  Swept 4..256 on every config: 32 is best everywhere (finer static
// ranges even out the tail; beyond 64 the per-block staging and the shorter ranges cost more than they give)
constexpr int kGridMultDefault = 32;
int grid_mult(const tinsel_hip* r) { return r->tune.grid_mult > 0 ? r->tune.grid_mult : kGridMultDefault; }

// the paired pipeline (tn_paired.h) takes flat-scan scenes without detail counting; anything else asked of it runs the split pipeline
bool paired_can(const tinsel_hip* r) { return r->scene.flatScan != 0 && !r->countDetail; }

// Where a path kernel that stages `staged` bytes of the arena into LDS finds the scene (SceneT, tn_scene.h): all of it in LDS (every mesh
// rides in the arena), the arena in LDS beside meshes in HBM (MIXED), or in HBM
enum Residency { RES_HBM, RES_LDS, RES_MIXED };
Residency residency(const DevScene& sc, uint32_t staged) { return sc.allInArena ? RES_LDS : (staged != 0 && staged == sc.arenaBytes) ? RES_MIXED : RES_HBM; }

// Which scan variants a scene gets (the W1 / W2 instances of tn_launch.h): 1 = every mesh primitive is walked by k_walk -- the lean kernels,
// compiled without the inline mesh walk; 2 = every mesh primitive is walked OR is a quad (one internal node over two triangles: a lamp, a card),
// which the scan tests with ray_mesh_two_leaves -- no stack, no loop -- where the arena is staged beside meshes in HBM (glass.tin: sphere and
// cube walked, the lamp a quad); 0 = some mesh is walked inline: the general kernels.
int walked_only_level(const tinsel_hip* r)
{
    const Residency res = residency(r->scene, r->scene.arenaLdsBytes);
    if (!r->walkEnabled || r->walkPrims.count == 0 || r->countDetail || res == RES_LDS)
        return 0;
    int meshPrims = 0, quads = 0;
    for (size_t i = 0; i < r->primMesh.size(); ++i)
    {
        const int m = r->primMesh[i];
        if (m < 0)
            continue;
        ++meshPrims;
        if (!(r->primsHost[i].flags & kPrimWalked) && r->meshesNow[(size_t)m].twoLeaves)
            ++quads;
    }
    if (meshPrims == r->walkPrims.count)
        return 1;
    if (r->tune.quads_in_scan != 0 && res == RES_MIXED && meshPrims == r->walkPrims.count + quads)
        return 2;
    return 0;
}

// AUTO's choice between the split pipeline and its paired re-cut, by what was measured (profiles/r06_h_ab_paired.md, Msamples/s split -> paired):
// k_step runs a path's shadow resolve, its closest hit and its shading in ONE kernel at four waves per SIMD, so it wins where all three are lean --
// every mesh walked by k_walk (the scan kernels' WONLY variants: no inline mesh walk, no deep stack), nothing moving (no pose interpolated per ray),
// lights that are sampled without a search (spheres, a probe, small meshes): the 524k-triangle config 2232 -> 2536, the Aphrodite scan 2865 -> 3290,
// transmission.tin 1211 -> 1338 -- and is a wash or loses elsewhere: glass 1613 -> 1608 and table.tin 1323 -> 1307 (a mesh walked inline),
// motionblur 1488 -> 1410 (a moving mesh), meshlight.tin 1471 -> 1380 (a 36,752-triangle light: a CDF search per sample).
bool paired_preferred(const tinsel_hip* r)
{
    // (level 2 -- a quad tested in the scan beside the walked meshes, glass.tin -- stays with the split pipeline: 1662 against 1601 Msamples/s,
    // profiles/r06_2d_ab_glass.md; its k_step is not short of registers any more, it has 2x the instructions per path-step of the 524k-triangle config's)
    if (!paired_can(r) || r->walkPrims.count == 0 || !r->walkEnabled || walked_only_level(r) != 1)
        return false;
    for (const Prim64& p : r->primsHost)
        if (p.flags & kPrimMoving)
            return false;
    for (int32_t i : r->lightPrims)
        if (r->primMesh[(size_t)i] >= 0 && r->meshesNow[(size_t)r->primMesh[(size_t)i]].numTris > 64)
            return false;
    return true;
}

int resolve_pipeline(const tinsel_hip* r)
{
    if (r->pipeline == TINSEL_PIPELINE_WAVEFRONT_PAIRED)
        return paired_can(r) ? TINSEL_PIPELINE_WAVEFRONT_PAIRED : TINSEL_PIPELINE_WAVEFRONT_SPLIT;
    if (r->pipeline == TINSEL_PIPELINE_AUTO && !r->scene.allInArena && paired_preferred(r))
        return TINSEL_PIPELINE_WAVEFRONT_PAIRED;
    if (r->pipeline != TINSEL_PIPELINE_AUTO)
        return r->pipeline;
    // A scene whose arena is staged whole into LDS runs the fused kernel, whatever its shadow rays per bounce (fused ->
    // split, Msamples/s: cornell 2550 -> 2055, gloss 6250 -> 4070, env_loft 3540 -> 2260, 4 rays: veach 1295 -> 1267, 9 rays:
    // features 690 -> 616, 10 rays: features + probe 589 -> 515; until the BSDF terms moved behind the shadow traces the
    // many-ray scenes were faster split); scenes with meshes or a scene BVH in HBM run the split pipeline.
    return r->scene.allInArena ? TINSEL_PIPELINE_WAVEFRONT : TINSEL_PIPELINE_WAVEFRONT_SPLIT;
}

// The pipeline of paths the CALLER starts (a radiance or a gather query): the paired pipeline where a render would run it, and the split pipeline
// in every other case -- also on a scene a render takes through the fused kernel, and under a MEGAKERNEL setting: k_bounce and k_mega make the
// camera's paths inside the kernel, the split and the paired pipeline in ONE kernel in front of everything else (k_generate), which
// k_generate_rays / k_generate_gather stand in for.
int radiance_pipeline(const tinsel_hip* r)
{
    return resolve_pipeline(r) == TINSEL_PIPELINE_WAVEFRONT_PAIRED ? TINSEL_PIPELINE_WAVEFRONT_PAIRED : TINSEL_PIPELINE_WAVEFRONT_SPLIT;
}

// CameraSampler constructor (util.h:45-71) + Mat44(Transform) (maths.h:841-849), host side, once per call
void make_camera(const tinsel_camera& c, int width, int height, CameraParams& out)
{
    // Mat33(Quat): columns are q*e_k (maths.h:654-663); Mat44(Transform): cols*s, translation p*s with s == 1
    Q4 q = { c.rotation.x, c.rotation.y, c.rotation.z, c.rotation.w };
    const float s = 1.0f;
    V3 c0 = qrotate(q, V3(1.0f, 0.0f, 0.0f))*s;
    V3 c1 = qrotate(q, V3(0.0f, 1.0f, 0.0f))*s;
    V3 c2 = qrotate(q, V3(0.0f, 0.0f, 1.0f))*s;
    V3 c3 = V3(c.position.x, c.position.y, c.position.z)*s;

    // column-major 4x4s
    float c2w[16] = { c0.x, c0.y, c0.z, 0.0f, c1.x, c1.y, c1.z, 0.0f, c2.x, c2.y, c2.z, 0.0f, c3.x, c3.y, c3.z, 1.0f };

    // rasterToScreen given row-wise in the reference constructor (maths.h:801-829)
    float r2s[16] = { 2.0f/width, 0.0f, 0.0f, 0.0f,
                      0.0f, -2.0f/height, 0.0f, 0.0f,
                      0.0f, 0.0f, 1.0f, 0.0f,
                      -1.0f, 1.0f, 1.0f, 1.0f };

    float f = tanf(c.fov*0.5f);
    float aspect = float(width)/height;

    float s2c[16] = { f*aspect, 0.0f, 0.0f, 0.0f,
                      0.0f, f, 0.0f, 0.0f,
                      0.0f, 0.0f, -1.0f, 0.0f,
                      0.0f, 0.0f, 0.0f, 1.0f };

    // MatrixMultiply<4,4,4> (maths.h:83-99): result[i+j*4] = sum_k a[i+k*4]*b[k+j*4], k ascending from t = 0
    auto mul = [](float* result, const float* a, const float* b) {
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j)
            {
                float t = 0.0f;
                for (int k = 0; k < 4; ++k)
                    t += a[i + k*4]*b[k + j*4];
                result[i + j*4] = t;
            }
    };

    float tmp[16];
    mul(tmp, c2w, s2c);             // cameraToWorld*screenToCamera
    mul(out.r2w, tmp, r2s);         // ... *rasterToScreen
    out.ox = c2w[12]; out.oy = c2w[13]; out.oz = c2w[14];
    out.shutterStart = c.shutter_start;
    out.shutterEnd = c.shutter_end;
}

// a timing event out of the pool (a new one where the pool is empty)
Event get_event(tinsel_hip* r)
{
    Event e;
    if (!r->eventPool.empty())
    {
        e = std::move(r->eventPool.back());
        r->eventPool.pop_back();
    }
    else
        (void)e.create(true);
    return e;
}

struct ScopedTimer
{
    tinsel_hip* r;
    hipStream_t stream;
    TimedSpan span;
    bool on;
    ScopedTimer(tinsel_hip* r_, int kernel, hipStream_t s) : r(r_), stream(s), on(r_->timing)
    {
        if (on)
        {
            span.kernel = kernel;
            span.start = get_event(r);
            span.stop = get_event(r);
            (void)hipEventRecord(span.start, stream);
        }
    }
    ~ScopedTimer()
    {
        if (on)
        {
            (void)hipEventRecord(span.stop, stream);
            r->spans.push_back(std::move(span));
        }
    }
};

int pick_stack(int need)
{
    const int sizes[] = { 8, 12, 16, 24, 32, 48, 64, 96, 128, 156 };
    for (int s : sizes)
        if (need <= s)
            return s;
    return -1;
}

// LDS per workgroup of traversal stacks `stack` deep (+ the staged arena)
size_t stack_bytes(const tinsel_hip* r, int stack) { return ((size_t)stack*kBlock + kScanWords)*sizeof(uint32_t) + r->scene.arenaLdsBytes; }
size_t stack_bytes(const tinsel_hip* r) { return stack_bytes(r, r->stackNeed); }

// The path kernels exist twice (tn_launch.h): this translation unit's, bit-identical to the CPU oracle, and
// tinsel_fast.hip's, built under the tolerance contract.  tinsel_hip_set_arithmetic picks the arm.
extern "C" int tinsel_fast_launch_path_kernel(const void* launchArgs, void* stream);
extern "C" int tinsel_fast_prepare_path_kernels(int sharedMemLimit, const char** first);
extern "C" unsigned tinsel_fast_launch_args_size(void);
extern "C" void tinsel_fast_launch_leaf(const void* leafArgs, void* stream);
extern "C" unsigned tinsel_fast_leaf_args_size(void);

// Raises the dynamic-LDS limit of every kernel that needs more than the default launch limit, for both arithmetic arms (tn_launch.h).  Called by
// tinsel_hip_create, which falls back to planning within 64 KB per workgroup when the runtime refuses a kernel (r->prepRefused: "kernel name (arm)").
void prepare_kernels_once(tinsel_hip* r)
{
    if (r->pathKernelsPrepared)
        return;
    const PrepReport rep = prepare_path_kernels(r->sharedMemLimit);
    r->segPrefixLds = rep.segPrefixLds;
    const char* fastFirst = nullptr;
    const int fastRefused = tinsel_fast_prepare_path_kernels(r->sharedMemLimit, &fastFirst);
    if (rep.refused)
        r->prepRefused = std::string(rep.first ? rep.first : "?") + " (parity arm; " + std::to_string(rep.refused + fastRefused) + " kernels in all)";
    else if (fastRefused)
        r->prepRefused = std::string(fastFirst ? fastFirst : "?") + " (tolerance arm; " + std::to_string(fastRefused) + " kernels in all)";
    r->pathKernelsPrepared = true;
}

int launch_path(tinsel_hip* r, const LaunchArgs& a, hipStream_t st)
{
    prepare_kernels_once(r);
    const bool ok = r->arith == TINSEL_ARITH_FAST ? tinsel_fast_launch_path_kernel(&a, st) == 0 : launch_path_kernel(a, st);
    return ok ? 0 : fail("launch: no path-kernel instance " + std::to_string(a.variant));
}

// What a launch record starts from: zero, the scene in force, traversal stacks of the scene's planned depth and the LDS they take
LaunchArgs launch_base(const tinsel_hip* r)
{
    LaunchArgs a;
    memset(&a, 0, sizeof(a));
    a.scene = r->scene;
    a.stackEntries = r->stackNeed;
    a.ldsBytes = (uint32_t)stack_bytes(r);
    return a;
}

// What cutting a batch into regions depends on (streaming_grid, cut_regions): plain values, no renderer
struct RegionSpec
{
    int numCUs = 256;
    int gridMult = kGridMultDefault;
    int K = 0;                          // shadow rays per path (tinsel_hip::neePerPath)
    bool fused = false;                 // k_bounce's batch; the split and paired pipelines keep their regions alike (cut_regions)
    int resident = kBounceWaves;        // k_bounce's workgroups resident per CU (plan_bounce)
    size_t maxRegions = 0;              // what the lane's arrays hold: regions (max_regions) and positions (DenseLane::splitCap)
    size_t capacity = 0;
    int tailSplit = -1, tailDivide = 4; // tinsel_hip_tuning::tail_split / tail_share / tail_divide
    float tailShare = 0.0f;
};

// how a batch is cut (SplitState::numRegions .. shortLen); a launch gives each group of four regions a workgroup of its own
struct RegionCut
{
    uint32_t numRegions = 0, regionLen = 0, bigRegions = 0, shortLen = 0;
    int grid() const { return (int)(numRegions/(kBlock/kWave)); }
};

// (half as many again as the widest grid: the short regions at the end of a batch, split_tail_regions)
size_t max_regions(int numCUs, int gridMult) { return (size_t)numCUs*(size_t)gridMult*(kBlock/kWave)*3/2; }

RegionSpec region_spec(const tinsel_hip_tuning& t, int numCUs, int K, bool fused, int resident)
{
    RegionSpec s;
    s.numCUs = numCUs;
    s.gridMult = t.grid_mult > 0 ? t.grid_mult : kGridMultDefault;
    s.K = K;
    s.fused = fused;
    s.resident = resident;
    s.maxRegions = max_regions(numCUs, s.gridMult);
    s.tailSplit = t.tail_split;
    s.tailShare = t.tail_share;
    s.tailDivide = t.tail_divide;
    return s;
}

// Blocks of the streaming kernels' grid = a quarter of the regions the batch is cut into (one region per wave, SplitState,
// tn_kernels.h).  A wave works through its region 64 entries at a time and a round is as long as its slowest lane, so
// regions should stay long as paths die (the last round of a region is the ragged one), yet there must be enough of them to
// balance: ~1024 positions per region, between 2 and 32 blocks per CU.  Fused kernel, cornell: a 1 M-path batch 1417 / 1520 /
// 1655 / 1747 Msamples/s at 16 / 8 / 4 / 2 blocks per CU (regions of 64 ... 512); a 64 Mi batch 2644 / 2735 / 2803 at 8 / 16 /
// 32 (regions of 8192 / 4096 / 2048).
int streaming_grid(const RegionSpec& s, size_t slots)
{
    // (where the fused kernel's waves share their workgroup's regions -- three or more shadow rays per bounce, k_bounce -- the
    // regions may be twice as long: features 707 -> 740, features + probe 595 -> 622, veach +-0)
    const size_t regionTarget = (s.fused && s.K >= 3) ? 2048 : 1024;
    const size_t perBlock = regionTarget*(kBlock/kWave);
    const size_t blocks = (slots + perBlock - 1)/perBlock;
    // (at least as many workgroups as the chip holds at once -- k_bounce's resident workgroups per CU, three for the split pipeline's kernels --
    // where the batch has that many 256-path pieces: a 1 M-path batch would otherwise leave the last wave slot empty)
    const int gridMin = s.fused ? s.resident : 3;
    const size_t lo = std::min<size_t>((size_t)s.numCUs*(size_t)gridMin, (slots + kBlock - 1)/kBlock), hi = (size_t)s.numCUs*(size_t)s.gridMult;
    size_t grid = std::max<size_t>(1, std::min(hi, std::max(lo, blocks)));
    // The workgroups that HAVE work (regions are a whole number of waves long, so fewer than the grid may) as close to a whole number
    // of resident sets (gridMin per CU) as the region length allows within +-25 %: the last set of a launch is then full instead
    // of, say, two thirds empty.  Glass at 20 passes per batch 1262 -> 1291 Msamples/s, the 524k-triangle config 2024 -> 2034, the
    // fused configs +-0 (profiles/r03_s_ab_grid_round.txt)
    const size_t resident = (size_t)s.numCUs*(size_t)gridMin;
    if (grid > 2*resident)
    {
        auto busy = [&](size_t g) {         // workgroups with work for a grid of g (set_regions' region length)
            const size_t regions = g*(kBlock/kWave);
            const size_t len = ((slots + regions - 1)/regions + kWave - 1)/kWave*kWave;
            return (slots + len*(kBlock/kWave) - 1)/(len*(kBlock/kWave));
        };
        size_t best = grid;
        double bestWaste = 2.0;
        for (size_t g = std::max(grid*3/4, 2*resident); g <= std::min(hi, grid*5/4); g += std::max<size_t>(1, resident/16))
        {
            const size_t b = busy(g);
            const double sets = (double)b/(double)resident;
            const double waste = std::ceil(sets) - sets;        // empty fraction of the last resident set
            if (waste < bestWaste - 1e-9)
            {
                bestWaste = waste;
                best = g;
            }
        }
        grid = best;
    }
    return (int)grid;
}

// `grid` region groups, all alike; false where the lane's arrays cannot hold them
bool set_regions(const RegionSpec& s, size_t slots, int grid, RegionCut& c)
{
    c.numRegions = (uint32_t)grid*(kBlock/kWave);
    c.regionLen = (uint32_t)(((slots + c.numRegions - 1)/c.numRegions + kWave - 1)/kWave*kWave);
    c.bigRegions = c.numRegions;
    c.shortLen = c.regionLen;
    return c.numRegions <= s.maxRegions && (size_t)c.numRegions*c.regionLen <= s.capacity;
}

// The last `tailShare` of the batch's positions in regions 1/divide as long (SplitState::bigRegions / shortLen, tn_kernels.h): what the chip
// works on when a launch runs out.  The region arrays bound their number: where the uniform cut is already at the bound the long regions get
// longer.  Leaves `c` as set_regions made it when the batch is too small for any of that.
void split_tail_regions(const RegionSpec& s, RegionCut& c, size_t slots, double tailShare, int divide)
{
    const uint32_t per = kBlock/kWave;                        // regions per group
    const size_t maxRegions = s.maxRegions;
    if (c.regionLen < (uint32_t)(kWave*divide*2) || c.numRegions < 64u*per || maxRegions < 128u*per)
        return;
    const double factor = (1.0 - tailShare) + tailShare*(double)divide;
    uint32_t L = c.regionLen;
    if ((double)slots*factor/(double)L + 2.0*per > (double)maxRegions)
        L = (uint32_t)(((size_t)((double)slots*factor/(double)(maxRegions - 2*per)) + kWave)/kWave*kWave);
    const uint32_t S = L/(uint32_t)divide/kWave*kWave;        // short regions: a multiple of 64 positions
    const uint32_t big = (uint32_t)((double)slots*(1.0 - tailShare)/(double)L)/per*per;
    const size_t covered = (size_t)big*L;
    if (S < (uint32_t)kWave || big < per || covered >= slots)
        return;
    const size_t rest = slots - covered;
    const uint32_t small = (uint32_t)((rest + (size_t)S*per - 1)/((size_t)S*per))*per;
    if (big + small > maxRegions || (size_t)big*L + (size_t)small*S > s.capacity)
        return;
    c.regionLen = L;
    c.bigRegions = big;
    c.shortLen = S;
    c.numRegions = big + small;
}

// A batch that ONE resident set of workgroups takes whole (cfg1: 256^2 x 16 passes = 683 region groups for 768 slots): two thirds of the CUs
// get three groups, a third gets two, and the launch lasts as long as three.  Cut so that every CU gets TWO long groups -- three quarters of
// the batch -- and the rest in groups a third as long, which the dispatcher deals out as slots come free: every CU ends up with the same
// work.  cornell 256^2 x 16 passes 2402 -> 2670 Msamples/s, 512^2 x 4 2600 -> 2919, veach 256^2 x 16 1176 -> 1324 (call Z10).
bool split_one_set(const RegionSpec& s, RegionCut& c, size_t slots)
{
    const uint32_t per = kBlock/kWave;
    const size_t cus = (size_t)s.numCUs;
    // (W workgroups resident per CU: W - 1 long groups per CU hold W/(W + 1) of the batch -- three waves: two groups, three quarters)
    const size_t W = (size_t)s.resident;
    if (W < 2)
        return false;
    const uint32_t L = (uint32_t)((slots*W/(W + 1))/((W - 1)*cus*per)/kWave*kWave);
    if (L < 3u*kWave)
        return false;
    const uint32_t S = L/3/kWave*kWave;
    const uint32_t big = (uint32_t)((W - 1)*cus)*per;
    const size_t covered = (size_t)big*L;
    if (covered >= slots)
        return false;
    const uint32_t small = (uint32_t)((slots - covered + (size_t)S*per - 1)/((size_t)S*per))*per;
    if (big + small > s.maxRegions || (size_t)big*L + (size_t)small*S > s.capacity)
        return false;
    c.regionLen = L;
    c.bigRegions = big;
    c.shortLen = S;
    c.numRegions = big + small;
    return true;
}

// set_regions + the short regions at the end.  The last eighth or so of the positions in regions a quarter as long: a workgroup's region group
// is 0.75 ms of a 5 ms launch (cornell, 20 passes) and a launch ends when its last workgroup does.  k_bounce alone (round 3, call Z5):
// cornell 1024^2 x 20 passes 3878 -> 4012 Msamples/s, x 8 3539 -> 3685, 512^2 x 16 2812 -> 3021, features 1183 -> 1292, veach 1080p
// 2414 -> 2610 (profiles/r03_z5_ab_tail_split.md).  tinsel_hip_tuning::tail_split / tail_share / tail_divide (A/B).  The cut's grid() is
// the number of region groups = the workgroups of a launch that gives every group its own.  False where the lane's arrays cannot hold the batch.
bool cut_regions(const RegionSpec& s, size_t slots, int grid, RegionCut& c)
{
    if (!set_regions(s, slots, grid, c))
        return false;
    // No short regions at the end for the split and paired pipelines: the launches are many and short, k_walk cuts its
    // own list into static ranges, and more regions cost k_seg_prefix / k_walk more than the other kernels' tails gain -- the 524k-triangle
    // config 2319 -> 2254 Msamples/s, many_spheres 2108 -> 2082, glass +-0 (profiles/r03_z5_ab_tail_split.md).
    if (!s.fused)
        return true;
    double share = -0.5;
    int divide = 4;
    if (s.tailSplit == 0)
        share = 0.0;
    else if (s.tailSplit > 0)
    {
        share = (double)s.tailShare;
        divide = s.tailDivide;
    }
    // (s.resident workgroups per CU are resident: plan_bounce)
    if (share < 0.0 && (size_t)grid <= (size_t)s.numCUs*s.resident && (size_t)grid > (size_t)s.numCUs*(s.resident - 1) && split_one_set(s, c, slots))
        return true;
    if (share < 0.0)
    {
        // a negative share: that multiple of ONE resident set's part of the batch (s.resident workgroups per CU).  The default, half a
        // set's part, against a fixed eighth: cornell x 20 passes 4036 -> 4059, x 64 4203 -> 4221, features 1289 -> 1298, veach 1080p
        // 2610 -> 2621, gloss 10570 -> 10530 (call Z8)
        const double sets = (double)grid/(double)(s.resident*s.numCUs);
        share = std::min(0.25, std::max(0.03, -share/std::max(1.0, sets)));
    }
    if (share > 0.0 && share < 0.9 && divide >= 2)
        split_tail_regions(s, c, slots, share, divide);
    return true;
}

// k_bounce's LDS plan for the scene: does it close ranks through the waves' shading pools (returned)?  Pools (25 KB of LDS per workgroup)
// where rays can LEAVE the scene -- veach 1515 -> 1866 Msamples/s, features 755 -> 865, env_loft 3598 -> 3793, gloss 7584 -> 7934 when they
// were introduced; between two facing planes every ray hits something and the pools only cost (cornell 2919 -> 2894) -- and where they do not
// cost the third resident workgroup (features' 32-KB arena + pools would leave two).  The kernel runs four waves per SIMD = four workgroups
// per CU by its registers (kBounceWaves); *resident, which the grid and the region cut are sized by, is what the LDS lets be resident.
bool plan_bounce(const tinsel_hip* r, int* resident)
{
    const size_t perCU = 160u*1024u;
    const size_t lds = stack_bytes(r), withPool = lds + kPoolWords*sizeof(uint32_t);
    const bool want = r->tune.repack >= 0 ? r->tune.repack != 0 : !r->sceneEnclosed;      // tinsel_hip_tuning::repack 0 / 1: never / always; default: open scenes
    const bool pools = want && withPool*3 <= perCU && withPool <= (size_t)r->sharedMemLimit;
    // the workgroups per CU the grid and the region cut are sized by = the ones that ARE resident: four by the registers, fewer where a
    // workgroup's LDS (stacks + staged arena + pools) says so (with pools, three fit where four times their LDS do not)
    const size_t ldsPerGroup = std::max<size_t>(1, pools ? withPool : lds);
    *resident = (int)std::max<size_t>(1, std::min<size_t>((size_t)kBounceWaves, perCU/ldsPerGroup));
    return pools;
}

// What the scene as it is now and a render's plan ask of the fused kernel (BounceFeature, tn_scene.h), but for kFeatShare, which the cut of
// each batch decides (trace_fused).  Derived for every render call, from what the host holds of the scene in force: a moved primitive, a
// rebuilt mesh tree, another tuning or roulette setting cannot leave a stale set behind.
uint32_t bounce_features(const tinsel_hip* r, bool pools)
{
    uint32_t f = 0;
    f |= r->scene.hasMedia ? kFeatMedia : 0u;
    f |= r->scene.probe.valid ? kFeatProbe : 0u;
    f |= r->anyTransmission ? kFeatTransmission : 0u;
    f |= r->scene.sortQueues ? kFeatSort : 0u;
    f |= pools ? kFeatPools : 0u;
    f |= r->rrStart > 0 ? kFeatRoulette : 0u;
    for (size_t i = 0; i < r->primsHost.size(); ++i)
    {
        const Prim64& p = r->primsHost[i];
        f |= (p.flags & kPrimMoving) ? kFeatMotion : 0u;
        f |= p.type == (uint32_t)kPrimSphere ? kFeatSphere : 0u;
        const int m = i < r->primMesh.size() ? r->primMesh[i] : -1;
        if (p.type == (uint32_t)kPrimMesh && !(p.flags & kPrimQuadArena) && !(m >= 0 && r->meshesNow[(size_t)m].twoLeaves))
            f |= kFeatMeshWalk;
    }
    return f;
}

// Do the scene's paths carry the SLIM state (load_state_slim, tn_path_state.h)?  What the slim state has no word for -- a medium, a ray
// time, a transmitted or specular ray type, a probe's MIS -- and what the FIT sets leave out anyway (a walked mesh), among the scene's own
// bits of `features`; and no subsurface: every material's is +0.0f by its bits (`anySubsurface`).  Every FIT instance is compiled slim, so
// this is one more condition of theirs (plan_batch); the feature bits themselves do not know about subsurface.  Derived for every
// render call like they are; tinsel_hip_scene_slim states it from a scene description.
bool scene_slim(uint32_t features, bool anySubsurface)
{
    return !(features & (kFeatMedia | kFeatProbe | kFeatMotion | kFeatMeshWalk | kFeatTransmission)) && !anySubsurface;
}

// the FIT instance of k_bounce (tn_launch.h) for a scene whose features are `need`, PK_NONE where none is compiled for them
int fit_bounce(uint32_t need, bool deferMeshes)
{
    auto within = [&](int kind) { return (need & ~bounce_kind_features(kind)) == 0u; };
    if (deferMeshes)
        return within(kBounceFitDeferred) ? PK_BOUNCE_FIT_DEFERRED : PK_NONE;
    return within(kBounceFitClosed) ? PK_BOUNCE_FIT_CLOSED : PK_NONE;
}

// Would a camera render's plan give this scene the closed FIT instance (plan_batch below: the fused pipeline, the whole scene in LDS, the flat
// scan, no detail counters, bounce_fit on, a slim scene whose features lie inside the closed set, no deferred walks)?  `why`: the first
// condition that fails.  This is the rule a baked instance is offered by (tinsel_hip_bake_source).
bool plans_fit_closed(const tinsel_hip* r, std::string* why)
{
    auto no = [&](const char* w) { if (why) *why = w; return false; };
    if (resolve_pipeline(r) != TINSEL_PIPELINE_WAVEFRONT)
        return no("the scene does not run the fused pipeline");
    if (residency(r->scene, r->scene.arenaLdsBytes) != RES_LDS)
        return no("the scene is not staged whole into LDS");
    if (r->countDetail)
        return no("detail counters are on");
    if (!r->scene.flatScan)
        return no("the scene level is not a flat scan");
    if (r->tune.bounce_fit == 0)
        return no("tinsel_hip_tuning::bounce_fit is 0");
    int resident = 0;
    const uint32_t need = bounce_features(r, plan_bounce(r, &resident));
    if (!scene_slim(need, r->anySubsurface))
        return no("the scene is not slim (a medium, a probe, motion, a walked mesh, transmission or subsurface)");
    if (fit_bounce(need, r->scene.deferMeshes != 0) != PK_BOUNCE_FIT_CLOSED)
        return no(r->scene.deferMeshes ? "the scene defers its mesh walks (the deferred FIT instance is not baked)" : "the scene's features lie outside the closed FIT set");
    return true;
}

// Does the installed baked function serve this launch of PK_BOUNCE_FIT_CLOSED?  Only the exact arithmetic arm, only within the dynamic LDS
// the function may ask for, and only where its key is the key of the scene level in force NOW
bool baked_serves(const tinsel_hip* r, const LaunchArgs& a)
{
    return r->baked.fn != nullptr && r->baked.mode != 0 && r->arith == TINSEL_ARITH_EXACT && a.ldsBytes <= r->baked.ldsLimit &&
           r->baked.key == bake_live_key(r);
}

// k_walk's launches of a render call (plan_walk): instance, workgroup, workgroups per CU, dynamic LDS, the job's fixed part
struct WalkPlan
{
    int variant = PK_NONE, block = 256, perCU = 1;
    bool single = false;                // ONE walked primitive: k_walk; else k_walk_rays (a work item is a ray)
    uint32_t ldsBytes = 0;
    WalkJob job = {};
};

// k_swalk's launches (plan_swalk): as WalkPlan, an instance per ray kind, and the arena bytes it stages (its scene.arenaLdsBytes)
struct SwalkPlan
{
    int extend = PK_NONE, shadow = PK_NONE, block = kBlock, perCU = 32;
    uint32_t ldsBytes = 0, arenaLds = 0;
    SwalkJob job = {};
};

// k_walk (tn_walk.h): closest hits of the front rays of a queue against the large meshes in HBM, ahead of the scan kernel.  One 1024-thread
// workgroup per CU whose LDS holds the traversal stacks and, in what is left of the 160 KB, the top of the walked trees; trees too deep for
// that (a device-built LBVH of 524k triangles: 48 entries per lane) run 256-thread workgroups without a staged top.
WalkPlan plan_walk(const tinsel_hip* r)
{
    const tinsel_hip_tuning& t = r->tune;
    WalkPlan w;
    WalkJob& job = w.job;
    // (measured and settled, profiles/EXPERIMENTS.md: one resident set of workgroups; a refill once 24 lanes idle; a triangle phase once 8 wait)
    const int gridMult = t.walk_grid_mult > 0 ? t.walk_grid_mult : 1;
    job.refillMin = std::min(64, std::max(1, t.walk_refill_min > 0 ? t.walk_refill_min : 24));
    job.leafMin = std::min(64, std::max(1, t.walk_leaf_min > 0 ? t.walk_leaf_min : 8));
    job.numPrims = r->walkPrims.count;
    job.prof = r->walkProf.get();
    int entries = 1;
    for (int k = 0; k < kWalkMaxPrims && k < r->walkPrims.count; ++k)
    {
        job.prim[k] = r->walkPrims.prim[k];
        entries = std::max(entries, r->meshesNow[(size_t)r->walkPrimMesh[k]].stackNeed);
    }
    // ONE walked primitive: its tree as kernel-argument scalars (tinsel_hip_tuning::walk_single = 0: per-lane pointers as for several; tests)
    w.single = r->walkPrims.count == 1 && t.walk_single != 0;
    // (k_walk_rays keeps one LDS entry per walked primitive behind its control words: tn_walk.h kWalkPrimWords)
    const size_t ctl = (kWalkCtlWords + (w.single ? 0 : kWalkMaxPrims*kWalkPrimWords))*sizeof(uint32_t);
    // n stack entries per lane in LDS (tinsel_hip_tuning::walk_lds_stack, default 8; 0: the deepest tree's need, one workgroup per CU), the
    // rest of the deepest tree's need in HBM, and TWO 1024-thread workgroups per CU (8 waves per SIMD at 64 VGPRs) sharing the CU's
    // LDS: the 524k-triangle config's k_walk 19.0 -> 16.6 ms per 32 passes (2042 -> 2199 Msamples/s; 6 entries 17.2, 12 entries 16.7),
    // glass 10.4 -> 9.9; results unchanged (a stack entry is a stack entry wherever it lives)
    const int ldsStackEnv = t.walk_lds_stack >= 0 ? t.walk_lds_stack : 8;
    const bool twoPerCU = ldsStackEnv > 0 && !t.walk_block;
    const int ldsEntries = twoPerCU ? std::min(entries, std::max(1, ldsStackEnv)) : entries;
    const int rows = w.single ? kWalkLaneRows : kWalkRayRows;      // (+ the per-lane rows, tn_walk.h)
    const size_t ldsBudget = twoPerCU ? (size_t)r->sharedMemLimit/2 : (size_t)r->sharedMemLimit;
    const bool big = t.walk_block ? t.walk_block == 1024 : (size_t)(ldsEntries + rows)*1024*sizeof(uint32_t) + ctl + 16384 <= ldsBudget;
    w.block = big ? 1024 : 256;
    size_t lds = (size_t)(ldsEntries + rows)*w.block*sizeof(uint32_t) + ctl;
    if (big)
    {
        // what is left of the CU's LDS goes to the tree tops, in primitive order
        size_t room = (ldsBudget - lds)/sizeof(Node64);
        for (int k = 0; k < r->walkPrims.count && room > 0; ++k)
        {
            const int n = (int)std::min<size_t>(room, (size_t)r->meshesNow[(size_t)r->walkPrimMesh[k]].topCount);
            job.topCount[k] = n;
            room -= (size_t)n;
            lds += (size_t)n*sizeof(Node64);
        }
    }
    w.ldsBytes = (uint32_t)lds;
    w.perCU = big ? gridMult*(twoPerCU ? 2 : 1) : gridMult*4;
    job.stackEntries = ldsEntries;
    job.overflowEntries = entries - ldsEntries;        // (the columns: ensure_walk_overflow)
    w.variant = w.single ? (!big ? PK_WALK_SINGLE_256 : twoPerCU ? PK_WALK_SINGLE_1024X2 : PK_WALK_SINGLE_1024)
                         : (!big ? PK_WALK_RAYS_256 : twoPerCU ? PK_WALK_RAYS_1024X2 : PK_WALK_RAYS_1024);
    return w;
}

// k_swalk (tn_swalk.h): 1024-thread workgroups with the whole arena beside their stacks where it fits (the whole scene in LDS, or MIXED where a
// mesh lives in HBM), else 256-thread ones with generic pointers (tinsel_hip_tuning::swalk_lds = 0: always)
SwalkPlan plan_swalk(const tinsel_hip* r)
{
    SwalkPlan s;
    s.job = { nullptr, nullptr, 0, r->stackNeed, 32, 16 };         // (refill / leaf phase at 32 / 16 lanes: profiles/r03_d_ab_swalk.txt, r03_e_ab_swalk.txt)
    const size_t bigLds = ((size_t)r->stackNeed*1024 + kSwalkCtlWords)*sizeof(uint32_t) + r->scene.arenaBytes;
    const bool big = r->tune.swalk_lds != 0 && bigLds <= (size_t)r->sharedMemLimit;
    const bool allInArena = std::all_of(r->meshesNow.begin(), r->meshesNow.end(), [](const DevMesh& m) { return m.inArena != 0; });
    s.extend = !big ? PK_SWALK_EXTEND : allInArena ? PK_SWALK_EXTEND_LDS : PK_SWALK_EXTEND_MIXED;
    s.shadow = !big ? PK_SWALK_SHADOW : allInArena ? PK_SWALK_SHADOW_LDS : PK_SWALK_SHADOW_MIXED;
    s.block = big ? 1024 : kBlock;
    s.perCU = big ? 1 : 32;
    s.arenaLds = big ? r->scene.arenaBytes : r->scene.arenaLdsBytes;
    s.ldsBytes = (uint32_t)(((size_t)r->stackNeed*s.block + kSwalkCtlWords)*sizeof(uint32_t) + s.arenaLds);
    return s;
}

// What a render call's batches run, decided once per call (plan_batch), each field from the ones before it: pipeline, overlap, capacity, k_walk,
// the scan kernels' stack and LDS, k_swalk, k_shade's arena and LDS, k_bounce's pools and resident workgroups, and the instance of every launch.
// render_impl, ensure_batch / alloc_dense, render_batch and the launch helpers read it; none decides again.
struct BatchPlan
{
    int pipeline = TINSEL_PIPELINE_MEGAKERNEL;
    // a batch of `slots` paths (ps.rad) traced as `lanes` chunks of at most chunkPasses passes, each in a lane of stateSlots paths
    int lanes = 1, chunkPasses = 1;
    size_t slots = 0, stateSlots = 0;
    // a lane's arrays (alloc_dense): positions, regions, shadow rays per path they hold (0: the fused kernel's, which keeps none)
    size_t capacity = 0, maxRegions = 0;
    int K = 0;
    // k_walk (split, paired): its records fit (allocated; `walkRays` rays per position), and it runs (not while the detail counters count the inline walk)
    bool walkRecords = false, walk = false;
    size_t walkRays = 0;
    // the scan kernels: stack entries (the scene level's only for the lean variants, walked_only_level), dynamic LDS
    int stackScan = 0;
    uint32_t ldsTrace = 0;
    // a walk list is allocated (k_walk's, or k_swalk's for scenes the flat scan cannot take): k_seg_prefix bounds the regions
    bool workList = false;
    bool sceneWalk = false;             // k_swalk in the place of k_extend / k_shadow (split)
    // split: the arena k_shade stages, the dynamic LDS of k_shade and k_lights
    uint32_t arenaLdsShade = 0, ldsShade = 0, ldsLights = 0;
    bool pools = false;                 // fused: k_bounce's shading pools (plan_bounce; its resident workgroups are regions.resident)
    RegionSpec regions;                 // how a batch is cut (render_batch bounds it by the lane's arrays)
    // the instance of each launch (tn_launch.h; PK_NONE: not launched -- k_lights where k_extend draws the light samples)
    int generate = PK_GENERATE, extend = PK_NONE, shadow = PK_NONE, lights = PK_NONE, shade = PK_NONE, step = PK_NONE, bounce = PK_NONE, mega = PK_NONE;
    // fused: the features asked of k_bounce (bounce_features), and its instance for a batch whose cut shares a workgroup's regions
    // (FrameParams::share, the one feature a batch's length decides: trace_fused takes `bounce` or `bounceShared`, nothing else)
    uint32_t bounceFeatures = 0;
    int bounceShared = PK_NONE;
    WalkPlan walkPlan;                  // where `walk`
    SwalkPlan swalkPlan;                // where `sceneWalk`
};

// perPass x perBatch paths per batch; mayOverlap: the batch may be traced as two chunks (not for a look-ahead, not for tinsel_hip_reserve);
// generate: the kernel that makes the batch's paths -- the camera's, or a query's, a views call's or a sample map's (PK_GENERATE_RAYS / _GATHER / _VIEWS / _SAMPLES), which run radiance_pipeline's choice;
// groups: a light-groups call's batch (tn_host_light_groups.h) -- the split pipeline whatever the setting, planned as a render's, with
// k_shade's GROUPS twin as its shading kernel (k_shade_sorted has none); SIDE_DEPTHS: a depth-planes call's (tn_host_depth_planes.h), the
// same with the DEPTHS twin
enum { SIDE_NONE = 0, SIDE_GROUPS, SIDE_DEPTHS };
BatchPlan plan_batch(const tinsel_hip* r, size_t perPass, int perBatch, bool mayOverlap, int generate = PK_GENERATE, int side = SIDE_NONE)
{
    const bool groups = side != SIDE_NONE;          // (what the plan makes of a side call: the split pipeline, k_shade's plain loop)
    BatchPlan p;
    p.generate = generate;
    p.pipeline = groups ? (int)TINSEL_PIPELINE_WAVEFRONT_SPLIT : generate == PK_GENERATE ? resolve_pipeline(r) : radiance_pipeline(r);
    const bool fused = p.pipeline == TINSEL_PIPELINE_WAVEFRONT, split = p.pipeline == TINSEL_PIPELINE_WAVEFRONT_SPLIT,
               paired = p.pipeline == TINSEL_PIPELINE_WAVEFRONT_PAIRED;

    // Overlapped chunks.  A batch of several passes can be traced as TWO chunks of passes on two streams, each with its own dense state
    // (a lane, ensure_batch), both writing their slots of the one radiance array; a chunk's accumulate kernel follows its own trace
    // on its own stream and the previous chunk's accumulate by an event -- the framebuffer adds keep the reference's pass order, so no
    // bit changes (tests/test_gpu_switches.py) -- and the two chunks' kernels fill each other's tails.  Measured built in
    // (profiles/r04_k_ab_overlap.md, Msamples/s off -> on): it pays where a bounce is MANY SHORT launches that leave the chip half empty
    // at their ends -- the scene-level walk of scenes beyond the flat scan (k_seg_* + k_swalk twice a bounce: many_spheres 2118 -> 2304)
    // -- and nowhere else: the fused kernel is one launch that already ends in short regions (cornell 1024^2 x 20 passes 4173 -> 4145,
    // x 256 4338 -> 4268, veach 4K 2838 -> 2846, gloss 10972 -> 10588, a 1 M-path batch 2748 -> 2406: two launches, two tails);
    // k_walk's workgroups take a CU's whole LDS and gain nothing from a neighbour (the 524k-triangle config 2223 -> 2114, glass 1426 ->
    // 1418).  (Two RENDERERS on two streams had looked like +4 % on cornell, profiles/r04_j_two_streams.txt: that was the host's
    // share of a call overlapping, not the device's.)  Default: scenes whose scene level is walked by k_swalk, batches of 8 Mi paths
    // or more.  tinsel_hip_tuning::overlap = 0 / 1: never / wherever a batch has two passes (A/B, tests).
    // (Decided before the capacity, so by the walk a scene asks for rather than by whether its records fit: walkRecords.)
    p.chunkPasses = perBatch;
    {
        const size_t minPaths = (size_t)8u << 20;
        const bool can = mayOverlap && perBatch >= 2 && p.pipeline != TINSEL_PIPELINE_MEGAKERNEL;
        const bool sceneWalked = split && !r->scene.flatScan && r->tune.scene_walk != 0 && !r->countDetail && !(r->walkPrims.count > 0 && r->walkEnabled);
        const bool want = r->tune.overlap >= 0 ? r->tune.overlap != 0 : (sceneWalked && perPass*(size_t)perBatch >= minPaths);
        if (can && want)
        {
            p.chunkPasses = (perBatch + 1)/2;
            p.lanes = 2;
        }
    }
    p.slots = perPass*(size_t)perBatch;
    p.stateSlots = perPass*(size_t)p.chunkPasses;

    p.K = (split || paired) ? r->neePerPath : 0;
    p.maxRegions = max_regions(r->numCUs, grid_mult(r));
    p.capacity = (p.stateSlots + p.maxRegions*kWave + kWave - 1)/kWave*kWave;      // a region is a whole number of waves long

    // k_walk: one 32-B closest hit per (ray, walked primitive), by position, fewer than 2^31 of them.  Split: extension and shadow rays share
    // the buffer (K rays per position, at least one); paired: K + 1 rays per position
    p.walkRays = split ? (size_t)std::max(p.K, 1) : (size_t)p.K + 1;
    p.walkRecords = (split || paired) && r->walkPrims.count > 0 && r->walkEnabled &&
                    (double)p.capacity*(double)p.walkRays*r->walkPrims.count < 2147483648.0;
    p.walk = p.walkRecords && !r->countDetail;

    const int wl = p.walk ? walked_only_level(r) : 0;          // the lean scan variants (W1 / W2)
    p.stackScan = wl ? std::max(1, pick_stack(r->sceneStackNeed)) : r->stackNeed;
    p.ldsTrace = (uint32_t)stack_bytes(r, p.stackScan);

    p.workList = p.walkRecords || (split && !r->scene.flatScan);
    // (not where k_walk does the walking: what is left for the scan kernels is too short for the two extra launches per
    // bounce to pay -- glass 1087 -> 1077, config 3 1891 -> 1881; many_spheres, scene BVH walked inline, 1168 -> 1290)
    // scenes the flat scan cannot take (more than 64 primitives): the scene-level walk with ray replacement (k_swalk, tn_swalk.h)
    // in the place of k_extend / k_shadow; the detail counters count the inline walks
    p.sceneWalk = split && r->tune.scene_walk != 0 && !r->scene.flatScan && !r->countDetail && !p.walk;

    // the lean k_extend draws the light samples itself, and so does the variant for a staged arena with meshes in HBM (glass): without the
    // SLP vectoriser it fits 128 VGPRs and saves k_lights' pass over the path state (k_extend 5.7 + k_lights 7.1 -> 11.2 ms per 32 passes,
    // glass 1366 -> 1425 Msamples/s; round 2, 170 VGPRs: 29.1 apart, 31.5 together; profiles/r03_k_ab_lights_in_extend.txt)
    const Residency res = residency(r->scene, r->scene.arenaLdsBytes);
    const bool lightsInMixed = split && !wl && !r->countDetail && res == RES_MIXED && !(r->tune.scene_walk != 0 && !r->scene.flatScan);
    const bool lightsDrawn = wl != 0 || lightsInMixed;
    // k_shade has no traversal stacks in LDS and reads a material per path: an arena too large to sit beside the stacks of the
    // trace kernels (32 KB) is still staged by it up to 60 KB (many_spheres, 39 KB of primitive and material records: k_shade
    // 7.8 -> 6.7 ms; staged in the trace kernels too it costs them their fourth wave per SIMD, 1380 -> 1280 Msamples/s, and
    // k_lights reads too little of it to repay the copy, 2.7 -> 3.1 ms)
    p.arenaLdsShade = (r->scene.arenaLdsBytes == 0 && r->scene.arenaBytes <= 61440u && r->tune.lds_scene != 0) ? r->scene.arenaBytes : r->scene.arenaLdsBytes;
    p.ldsShade = r->scene.allInArena ? r->scene.arenaBytes : p.arenaLdsShade;
    p.ldsLights = r->scene.allInArena ? r->scene.arenaBytes : r->scene.arenaLdsBytes;
    // k_shade_sorted takes a region's paths class by class (tn_kernels.h): chosen PER SCENE.  It pays where a good share of a
    // bounce's paths are rays that LEFT the scene (a cheap class that otherwise idles through its wave-mates' shading) and the
    // path state is not already ordered by k_walk's front / back split: many_spheres 2087 -> 2122 Msamples/s, and in the split
    // pipeline veach 1902 -> 2003, features 1047 -> 1093; it loses in an enclosed scene (glass: no ray leaves, 17.5 -> 19.3 ms) and
    // where k_walk runs (the 524k-triangle config 6.47 -> 6.86 ms) (profiles/r03_g_ab_shade_sorted.txt, r04_e_rates.md).
    // tinsel_hip_tuning::shade_sorted = 0 / 1 forces either arm (A/B, tests).
    const bool sorted = !groups && (r->tune.shade_sorted >= 0 ? r->tune.shade_sorted != 0 : (!r->sceneEnclosed && !p.walk)) &&
                        (size_t)p.ldsShade + kShadeListWords*sizeof(uint32_t) <= (size_t)r->sharedMemLimit;
    if (sorted)
        p.ldsShade += (uint32_t)(kShadeListWords*sizeof(uint32_t));

    int resident = kBounceWaves;
    if (fused)
        p.pools = plan_bounce(r, &resident);
    p.regions = region_spec(r->tune, r->numCUs, r->neePerPath, fused, resident);

    // the instances (tn_launch.h) by where the scene lives; the counting ones have no MIXED form (wl != 0: not counting, not all in LDS)
    const bool count = r->countDetail, lds = res == RES_LDS, mixed = !count && res == RES_MIXED,
               mixedShade = !count && residency(r->scene, p.arenaLdsShade) == RES_MIXED;
    p.extend = wl == 2 ? PK_EXTEND_W2_MIXED : wl && mixed ? PK_EXTEND_W1_MIXED : wl ? PK_EXTEND_W1 : lightsInMixed ? PK_EXTEND_MIXED_LIGHTS :
               mixed ? PK_EXTEND_MIXED : count ? (lds ? PK_EXTEND_COUNT_LDS : PK_EXTEND_COUNT) : lds ? PK_EXTEND_LDS : PK_EXTEND;
    p.shadow = wl == 2 ? PK_SHADOW_W2_MIXED : wl && mixed ? PK_SHADOW_W1_MIXED : wl ? PK_SHADOW_W1 :
               mixed ? PK_SHADOW_MIXED : count ? (lds ? PK_SHADOW_COUNT_LDS : PK_SHADOW_COUNT) : lds ? PK_SHADOW_LDS : PK_SHADOW;
    p.step = wl == 2 ? PK_STEP_W2_MIXED : wl && mixed ? PK_STEP_W1_MIXED : wl ? PK_STEP_W1 : mixed ? PK_STEP_MIXED : lds ? PK_STEP_LDS : PK_STEP;
    p.lights = lightsDrawn ? PK_NONE : mixed ? PK_LIGHTS_MIXED : lds ? PK_LIGHTS_LDS : PK_LIGHTS;
    p.shade = sorted ? (mixedShade ? PK_SHADE_SORTED_MIXED : lds ? PK_SHADE_SORTED_LDS : PK_SHADE_SORTED) : (mixedShade ? PK_SHADE_MIXED : lds ? PK_SHADE_LDS : PK_SHADE);
    if (side == SIDE_GROUPS)
        p.shade = p.shade == PK_SHADE_MIXED ? PK_SHADE_GROUPS_MIXED : p.shade == PK_SHADE_LDS ? PK_SHADE_GROUPS_LDS : PK_SHADE_GROUPS;
    if (side == SIDE_DEPTHS)
        p.shade = p.shade == PK_SHADE_MIXED ? PK_SHADE_DEPTHS_MIXED : p.shade == PK_SHADE_LDS ? PK_SHADE_DEPTHS_LDS : PK_SHADE_DEPTHS;
    // (the detail-counting variants walk the scene BVH: nothing to defer)
    p.bounce = count ? (lds ? PK_BOUNCE_COUNT_LDS : PK_BOUNCE_COUNT) : r->scene.deferMeshes ? (lds ? PK_BOUNCE_LDS_DEFER : PK_BOUNCE_DEFER) : lds ? PK_BOUNCE_LDS : PK_BOUNCE;
    p.bounceShared = p.bounce;
    if (fused)
    {
        // a FIT instance where one is compiled for what the scene and the plan ask for (the whole scene in LDS, the flat scan, no detail
        // counters: what every fused BASELINE scene is) and the scene is slim (no subsurface on top of the sets' own conditions: the
        // instances carry the slim path state); tinsel_hip_tuning::bounce_fit = 0: the general kernel (parity tests, A/B)
        p.bounceFeatures = bounce_features(r, p.pools);
        if (lds && !count && r->scene.flatScan && r->tune.bounce_fit != 0 && scene_slim(p.bounceFeatures, r->anySubsurface))
        {
            const int alone = fit_bounce(p.bounceFeatures, r->scene.deferMeshes != 0), shared = fit_bounce(p.bounceFeatures | kFeatShare, r->scene.deferMeshes != 0);
            p.bounce = alone != PK_NONE ? alone : p.bounce;
            p.bounceShared = shared != PK_NONE ? shared : p.bounceShared;
        }
    }
    p.mega = count ? (lds ? PK_MEGA_COUNT_LDS : PK_MEGA_COUNT) : lds ? PK_MEGA_LDS : PK_MEGA;
    p.walkPlan = p.walk ? plan_walk(r) : WalkPlan();
    p.swalkPlan = p.sceneWalk ? plan_swalk(r) : SwalkPlan();
    return p;
}

// The wavefront pipelines' state (SplitState, tn_kernels.h) of one lane: by POSITION, two buffers of everything a bounce rewrites; for the
// split pipeline also what its kernels hand to each other (hit, shadow rays and their results), for the paired one its light samples;
// k_walk's records and the walk list where the plan has them
int alloc_dense(tinsel_hip* r, const BatchPlan& p, tinsel_hip::DenseLane& lane, int maxDepth)
{
    const size_t K = (size_t)p.K, cap = p.capacity, maxRegions = p.maxRegions;
    SplitState& ss = lane.ss;
    memset(&ss, 0, sizeof(ss));
    for (int b = 0; b < 2; ++b)
        if (r->batchMem.alloc(&ss.rayO[b], cap) || r->batchMem.alloc(&ss.rayD[b], cap) || r->batchMem.alloc(&ss.thr[b], cap) ||
            r->batchMem.alloc(&ss.rad[b], cap) || r->batchMem.alloc(&ss.rngId[b], cap))
            return -1;
    if (r->batchMem.alloc(&ss.segFront, maxRegions*((size_t)maxDepth + 2)) || r->batchMem.alloc(&ss.segBack, maxRegions*((size_t)maxDepth + 2)) ||
        r->batchMem.alloc(&lane.regionOrder, maxRegions/(kBlock/kWave)) || r->batchMem.alloc(&lane.regionOrderNee, maxRegions/(kBlock/kWave)))
        return -1;
    ss.capacity = (uint32_t)cap;
    ss.neePerPath = (int32_t)K;
    lane.splitCap = cap;
    lane.splitMaxRegions = (uint32_t)maxRegions;
    if (p.pipeline == TINSEL_PIPELINE_WAVEFRONT_PAIRED)
    {
        // the K pending light samples of every path, by position, double-buffered like the state (tn_paired.h)
        for (int b = 0; b < 2; ++b)
            if (r->batchMem.alloc(&ss.pairThr[b], K ? cap : 1) || r->batchMem.alloc(&ss.pairRay[b], cap*K*2) || r->batchMem.alloc(&ss.pairPend[b], K > 1 ? cap*K*2 : cap))     // (sample k's two records at (2k, 2k + 1)*cap; sample 0 has no second one)
                return -1;
    }
    if (p.pipeline == TINSEL_PIPELINE_WAVEFRONT_SPLIT)
        if (r->batchMem.alloc(&ss.hit, cap) || r->batchMem.alloc(&ss.hitPrim, cap) || r->batchMem.alloc(&ss.pathNee, K ? cap : 1) ||
            r->batchMem.alloc(&ss.neeRay, cap*K*2) || r->batchMem.alloc(&ss.neeSky, r->scene.probe.valid ? cap : 1) ||
            r->batchMem.alloc(&ss.neeTime, K ? cap : 1) || r->batchMem.alloc(&ss.neeRes, cap*K) ||
            r->batchMem.alloc(&ss.neeFront, maxRegions*(size_t)maxDepth) || r->batchMem.alloc(&ss.neeBack, maxRegions*(size_t)maxDepth))
            return -1;
    if (p.walkRecords && r->batchMem.alloc(&lane.walkRec, cap*p.walkRays*(size_t)r->walkPrims.count*2))
        return -1;
    if (p.workList && (r->batchMem.alloc(&lane.walkList, cap) || r->batchMem.alloc(&lane.segPrefix, maxRegions + 1)))
        return -1;
    return 0;
}

// the batch buffers for a render call's plan: the radiance of p.slots paths, p.lanes lanes of dense state; kept where they hold the plan
// k_walk's stack entries beyond the LDS ones (WalkJob::overflow): columns for the widest grid of the plan (numCUs x perCU workgroups) in every
// lane, allocated with the batch: nothing is freed or allocated between the launches of a batch
int ensure_walk_overflow(tinsel_hip* r, const BatchPlan& p)
{
    const WalkPlan& w = p.walkPlan;
    const size_t need = p.walk ? (size_t)r->numCUs*(size_t)w.perCU*(size_t)w.block*(size_t)w.job.overflowEntries : 0;
    for (int k = 0; k < p.lanes && need; ++k)
    {
        DevBuf<uint32_t>& columns = r->walkOverflow[k];
        if (columns.count() >= need)
            continue;
        if (columns)
            (void)hipDeviceSynchronize();       // (another stream's launch may still use the old columns)
        if (columns.alloc(need))
            return fail("k_walk: no memory for the stack overflow");
    }
    return 0;
}

int ensure_batch(tinsel_hip* r, const BatchPlan& p, int maxDepth)
{
    if (ensure_walk_overflow(r, p))
        return -1;
    const int K = r->neePerPath;
    const tinsel_hip::DenseLane& lane = r->lane[0];
    if (r->batchSlots >= p.slots && r->batchStateSlots >= p.stateSlots && r->batchLanes >= p.lanes && r->batchNee == K && r->batchDepth >= maxDepth &&
        r->batchPipeline == p.pipeline && (lane.walkRec != nullptr) == p.walkRecords && (lane.walkList != nullptr) == p.workList)
        return 0;
    // (a radiance query's device entry, or look-ahead, may have left launches over the old buffers in flight on another stream)
    if (r->batchPipeline >= 0)
        HIP_TRY(hipDeviceSynchronize());
    free_batch(r);

    // the radiance of finished paths by slot is what every pipeline hands to the accumulate kernels
    PathState& ps = r->ps;
    memset(&ps, 0, sizeof(ps));
    if (r->batchMem.alloc(&ps.rad, p.slots))
        return -1;
    if (p.pipeline != TINSEL_PIPELINE_MEGAKERNEL)
        for (int k = 0; k < p.lanes; ++k)
            if (alloc_dense(r, p, r->lane[k], maxDepth))
                return -1;

    // slots of other shards are never written (gen_slot): keep their radiance at zero for the test hook
    HIP_TRY(hipMemset(ps.rad, 0, sizeof(float4)*p.slots));
    // (a memset of device memory only enqueues on the null stream, and the kernels that follow may run on a NON-BLOCKING stream
    // -- a group member's, the look-ahead's -- which the null stream does not order: without this wait the zeroes could land on
    // radiance a kernel had already written.  Allocation path only.)
    HIP_TRY(hipStreamSynchronize(nullptr));

    r->ctl.stats = r->statsDev.get();
    r->batchSlots = p.slots;
    r->batchStateSlots = p.stateSlots;
    r->batchLanes = p.lanes;
    r->batchNee = K;
    r->batchDepth = maxDepth;
    r->batchPipeline = p.pipeline;
    return 0;
}

// k_seg_prefix stages one count per region in dynamic LDS beside 64 B of static: what a launch may ask for (prepare_path_kernels raises
// the kernel's limit to the device's sharedMemLimit - 1024)
uint32_t seg_prefix_max_regions(tinsel_hip* r)
{
    prepare_kernels_once(r);
    return (uint32_t)std::max(0, r->segPrefixLds/4);
}

// k_seg_prefix's walk list visits the regions a golden-section step apart: every workgroup's static range gets the same mix of rays
// (k_walk's lesson; in k_swalk's index order a 256-thread grid of 8 workgroups per CU took 14.4 ms where 32 per CU took 9.2)
uint32_t seg_step(uint32_t numRegions)
{
    uint32_t step = (uint32_t)(numRegions*0.6180339887) | 1u;
    auto gcd = [](uint32_t x, uint32_t y) { while (y) { const uint32_t t = x % y; x = y; y = t; } return x; };
    while (step > 1 && gcd(step, numRegions) != 1)
        step -= 1;
    if (step >= numRegions || numRegions > 65535u)       // k_seg_prefix multiplies in 32 bits
        step = 1;
    return step;
}

// A walk's work list in lane L: k_seg_prefix over the regions, then their front entries (back == null: k_walk's paths / shadow-ray bundles
// whose ray enters a walked mesh's box) or every live entry, front and back (k_swalk's)
int work_list(tinsel_hip* r, const tinsel_hip::DenseLane& L, hipStream_t st, const LaunchArgs& a, const uint32_t* front, const uint32_t* back)
{
    const SplitState& ss = a.ss;
    ScopedTimer t(r, KN_SEG, st);
    if (ss.numRegions > seg_prefix_max_regions(r))
        return fail("k_seg_prefix: " + std::to_string(ss.numRegions) + " regions do not fit its LDS (tinsel_hip_tuning::grid_mult too large for this device)");
    hipLaunchKernelGGL(k_seg_prefix, dim3(1), dim3(kSegBlock), ss.numRegions*sizeof(uint32_t), st, front, back, ss.numRegions, seg_step(ss.numRegions), L.segPrefix);
    if (back)
        hipLaunchKernelGGL(k_seg_expand_all, dim3((unsigned)std::max(1, a.grid)), dim3(kBlock), 0, st, front, back, (const uint32_t*)L.segPrefix, ss, L.walkList);
    else
        hipLaunchKernelGGL(k_seg_expand, dim3((unsigned)std::max(1, a.grid)), dim3(kBlock), 0, st, front, (const uint32_t*)L.segPrefix, ss, L.walkList);
    return 0;
}

// k_walk (plan_walk) over the front rays of a queue.  (mixed: the paired pipeline's walk -- K shadow rays + the extension ray of every queued
// position, tn_paired.h.)  `slots`: the paths of the batch (or chunk) lane L traces
int launch_walk(tinsel_hip* r, const BatchPlan& p, tinsel_hip::DenseLane& L, hipStream_t st, LaunchArgs a, size_t slots, const uint32_t* regionCounts,
                bool shadowRays, bool mixed = false)
{
    const WalkPlan& w = p.walkPlan;
    const SplitState& ss = a.ss;
    if (work_list(r, L, st, a, regionCounts, nullptr))
        return -1;
    WalkJob& job = a.walk;
    job = w.job;
    job.queue = L.walkList;
    job.frontCount = L.segPrefix + ss.numRegions;
    job.rayO = ss.rayO[a.bounce & 1];
    job.rayD = ss.rayD[a.bounce & 1];
    const bool paired = p.pipeline == TINSEL_PIPELINE_WAVEFRONT_PAIRED;
    job.nee = paired ? ss.pairRay[a.bounce & 1] : ss.neeRay;
    job.neeStride = ss.capacity;
    job.neeTime = ss.neeTime;
    job.rec = L.walkRec;
    job.neePerPath = shadowRays ? r->neePerPath : 0;
    job.mixed = !paired ? 0 : mixed ? 1 : shadowRays ? 2 : 0;      // (2: shadow rays only, their time in the state: tn_walk.h)
    job.overflow = job.overflowEntries ? r->walkOverflow[&L - r->lane].get() : nullptr;
    // (a work item is a ray; with several walked primitives a lane keeps its ray as position | k << 27 while primitives are left: tn_walk.h)
    // (k_walk_rays, whatever the number of walked primitives: ADVICE r05)
    if (!w.single && (ss.capacity >= (1u << 27) || r->neePerPath >= 32))
        return fail("k_walk_rays: batch too large (>= 2^27 positions) or too many shadow rays per path (>= 32): lower tinsel_hip_tuning::batch_paths");
    const size_t items = slots*(size_t)((shadowRays && r->neePerPath > 1 ? r->neePerPath : 1) + (mixed ? 1 : 0));
    a.grid = (int)std::max<size_t>(1, std::min<size_t>((items + w.block - 1)/w.block, (size_t)r->numCUs*(size_t)w.perCU));
    a.variant = w.variant;
    a.ldsBytes = w.ldsBytes;
    ScopedTimer t(r, KN_WALK, st);
    return launch_path(r, a, st);
}

// k_swalk (plan_swalk): the scene-level walk with ray replacement, for scenes the flat scan cannot take.  The list: every live
// entry of every region (front and back), regions in index order -- the workgroups' static ranges are image patches, coherent rays.
int launch_swalk(tinsel_hip* r, const BatchPlan& p, const tinsel_hip::DenseLane& L, hipStream_t st, LaunchArgs a, size_t slots, const uint32_t* front,
                 const uint32_t* back, bool shadowRays)
{
    const SwalkPlan& w = p.swalkPlan;
    if (work_list(r, L, st, a, front, back))
        return -1;
    SwalkJob& job = a.swalk;
    job = w.job;
    job.list = L.walkList;
    job.count = L.segPrefix + a.ss.numRegions;
    job.neePerPath = shadowRays ? r->neePerPath : 0;
    const size_t items = slots*(size_t)(shadowRays && r->neePerPath > 1 ? r->neePerPath : 1);
    a.grid = (int)std::max<size_t>(1, std::min<size_t>((items + w.block - 1)/w.block, (size_t)r->numCUs*(size_t)w.perCU));
    a.scene.arenaLdsBytes = w.arenaLds;
    a.ldsBytes = w.ldsBytes;
    a.variant = shadowRays ? w.shadow : w.extend;
    ScopedTimer t(r, shadowRays ? KN_SHADOW : KN_EXTEND, st);
    return launch_path(r, a, st);
}

void launch_normals(tinsel_hip* r, hipStream_t st, int grid, const CameraParams& cam, const FrameParams& fp)
{
    if (r->scene.allInArena)
        hipLaunchKernelGGL((k_normals<true>), dim3(grid), dim3(kBlock), stack_bytes(r), st, r->scene, cam, fp, r->accum, r->stackNeed);
    else
        hipLaunchKernelGGL((k_normals<false>), dim3(grid), dim3(kBlock), stack_bytes(r), st, r->scene, cam, fp, r->accum, r->stackNeed);
}

// Accumulate tiles (16x16 pixels + filter halo) that contain at least one pixel owned by this shard; cached per
// (frame, shard, halo).  Ownership is a function of the pixel only (pixel_owned, tn_kernels.h).
int accumulate_tile_list(tinsel_hip* r, const FrameParams& fp)
{
    const int reachLo = 1 + (int)floorf(fp.filterWidth), reachHi = (int)ceilf(fp.filterWidth);
    const int key[6] = { fp.width, fp.height, fp.shardRank, fp.shardWorld, fp.shardTile, reachLo*16 + reachHi };
    if (r->accTilesDev && memcmp(key, r->accTilesKey, sizeof(key)) == 0)
        return 0;
    const int tilesX = (fp.width + kAccTile - 1)/kAccTile, tilesY = (fp.height + kAccTile - 1)/kAccTile;
    const int shardX = (fp.width + fp.shardTile - 1)/fp.shardTile;
    std::vector<std::pair<long long, int>> weighted;
    for (int ty = 0; ty < tilesY; ++ty)
    {
        for (int tx = 0; tx < tilesX; ++tx)
        {
            // candidate paths of this tile are generated at pixels [x0, x1] x [y0, y1]
            const int x0 = std::max(0, tx*kAccTile - reachLo), x1 = std::min(fp.width - 1, tx*kAccTile + kAccTile - 1 + reachHi);
            const int y0 = std::max(0, ty*kAccTile - reachLo), y1 = std::min(fp.height - 1, ty*kAccTile + kAccTile - 1 + reachHi);
            // ... of which this shard's: the rectangle cut with every shard tile it touches
            long long owned = 0;
            for (int sy = y0/fp.shardTile; sy <= y1/fp.shardTile; ++sy)
                for (int sx = x0/fp.shardTile; sx <= x1/fp.shardTile; ++sx)
                    if (((sy*shardX + sx) % fp.shardWorld) == fp.shardRank)
                        owned += (long long)(std::min(x1, sx*fp.shardTile + fp.shardTile - 1) - std::max(x0, sx*fp.shardTile) + 1)*
                                 (std::min(y1, sy*fp.shardTile + fp.shardTile - 1) - std::max(y0, sy*fp.shardTile) + 1);
            if (owned > 0)
                weighted.push_back({ -owned, ty*tilesX + tx });
        }
    }
    // the tiles with the most candidates first: a halo tile (a strip of a neighbouring shard tile's pixels) is a fraction of an inner
    // tile's work per pass (k_accumulate_tiled), and the launch ends in whatever was handed out last
    std::stable_sort(weighted.begin(), weighted.end(), [](const std::pair<long long, int>& a, const std::pair<long long, int>& b) { return a.first < b.first; });
    std::vector<int> list;
    for (const auto& w : weighted)
        list.push_back(w.second);
    DevBuf<int> tiles;
    if (tiles.upload(list.data(), list.size()))
        return -1;
    if (r->accTilesDev)
        HIP_TRY(hipDeviceSynchronize());        // (a launch in flight may still read the previous list)
    r->accTilesDev = std::move(tiles);
    r->accTilesCount = (int)list.size();
    memcpy(r->accTilesKey, key, sizeof(key));
    return 0;
}

// Paths resident per batch: 64 Mi for the wavefront pipelines (11 GB of path state of 288), 8 Mi for the megakernel arm.
// The split pipeline's trace launches end in a long tail (the slowest block of a deep traversal) and fewer, larger launches
// amortise it -- 524k-triangle config 765 / 941 / 992 Msamples/s at 8 / 32 / 64 Mi (round 1); the fused kernel wants its
// regions long (set_regions): cornell 2302 / 2803 Msamples/s at 8 / 64 Mi.  An explicit setting always wins.
size_t batch_slots(const tinsel_hip* r)
{
    if (!r->batchSlotsExplicit && r->pipeline != TINSEL_PIPELINE_MEGAKERNEL)
        return (size_t)64u << 20;
    return r->maxBatchSlots;
}

// Path slots one pass of this renderer's shard occupies: W*H for one shard, else its own tiles padded to full size.
size_t slots_per_pass(const tinsel_hip* r, int width, int height, int* tilesXOut = nullptr, int* ownedOut = nullptr)
{
    const int tilesX = (width + r->shardTile - 1)/r->shardTile;
    const int numTiles = tilesX*((height + r->shardTile - 1)/r->shardTile);
    const int owned = r->shardRank < numTiles ? (numTiles - r->shardRank + r->shardWorld - 1)/r->shardWorld : 0;
    if (tilesXOut) *tilesXOut = tilesX;
    if (ownedOut) *ownedOut = owned;
    if (r->shardWorld <= 1)
        return (size_t)width*height;
    return std::max<size_t>(1, (size_t)owned*r->shardTile*r->shardTile);
}

// Whole passes per batch of a call of `passes` under a limit of slotLimit path slots: one at least, however large a pass is
int passes_per_batch(size_t slotLimit, size_t perPass, int passes)
{
    return (int)std::min<size_t>((size_t)passes, std::max<size_t>(1, slotLimit/perPass));
}

// The support form of k_accumulate_tiled (tn_accumulate.h) adds nothing but what the full window adds when the filter's weight is +0 by
// construction from one pixel away on: Filter::Gaussian is max(0, expf(a) - offset) with a = -falloff*x*x, and for a <= argZero =
// log(offset) - 1e-6 (in double, rounded DOWN to float) e^a <= offset*(1 - 1e-6) while expf is off by less than an ulp (1.2e-7): the float
// expf(a) is below offset and the weight +0.  With falloff > 0 the argument falls with |x|, so -falloff*1*1 <= argZero puts every column a
// pixel or more from the sample there: of a path generated at pixel i, all but i and i + 1.  Widths up to 1 (the compile-time windows).
bool accumulate_support_rule(int filterType, float width, float falloff, float offset, float* argZero)
{
    *argZero = 0.0f;
    if (filterType == 0 || !(offset > 0.0f) || !std::isfinite(offset) || !(falloff > 0.0f) || !std::isfinite(falloff) || !(width > 0.0f) || !(width <= 1.0f))
        return false;
    const double z = std::log((double)offset) - 1e-6;
    float f = (float)z;
    if ((double)f > z)
        f = std::nextafterf(f, -INFINITY);
    *argZero = f;
    return -falloff*1.0f*1.0f <= f;
}

enum { ACC_FORM_UNTILED = 0, ACC_FORM_TILED, ACC_FORM_WIDE, ACC_FORM_PIPED, ACC_FORM_SUPPORT_TILED, ACC_FORM_SUPPORT_WIDE };

// Does the frame go through the tiled kernels (the footprint halo fits, 16-bit pixel coordinates)?
bool accumulate_tiled_fits(const FrameParams& fp)
{
    const int halo = 1 + (int)floorf(fp.filterWidth) + (int)ceilf(fp.filterWidth);
    return halo <= kAccMaxHalo && fp.filterWidth >= 0.0f && fp.width < 65536 && fp.height < 65536;
}

// What every tiled accumulate launch is given: `tiles` blocks (a shard: those of `tileList`); argZero: the support form's, else 0
struct AccLaunch { const uint32_t* passSeeds; const int* tileList; int tiles; hipStream_t st; PathState ps; const FrameParams& fp; float4* target; float argZero; };

// The compile-time windows (SPAN 3 and 4).  Which kernel (the same adds in the same order, tests/test_gpu_switches.py):
//   piped: staging of pass s + 1 overlapped with the gather of pass s (k_accumulate_piped: the launch is as long as one tile's pass loop;
//     cornell 256^2 x 16 passes 0.053 -> 0.037 ms, profiles/r05_q_ab_acc_piped.md; at 1024 tiles 0.100 -> 0.107, one shard of 8 of cornell
//     1024^2 0.565 -> 0.525 at 64-pixel tiles but 0.563 -> 0.613 at 32: not used there);
//   wide: 512-thread workgroups, the second half only stages (profiles/r03_y_ab_acc_wide.md);
//   else 256-thread workgroups.
// SUPPORT: the support form of the two k_accumulate_tiled launches; k_accumulate_piped has no such form.  Returns the form it ran.
template <int SPAN, bool SUPPORT>
int launch_accumulate_span(const AccLaunch& a, bool piped, bool wide)
{
    if (piped)
    {
        hipLaunchKernelGGL((k_accumulate_piped<SPAN>), dim3(a.tiles), dim3(kAccPipeThreads), 0, a.st, a.ps, a.fp, a.target, a.passSeeds, a.tileList);
        return ACC_FORM_PIPED;
    }
    if (wide)
    {
        hipLaunchKernelGGL((k_accumulate_tiled<SPAN, 2*kBlock, SUPPORT>), dim3(a.tiles), dim3(2*kBlock), 0, a.st, a.ps, a.fp, a.target, a.passSeeds, a.tileList, a.argZero);
        return SUPPORT ? ACC_FORM_SUPPORT_WIDE : ACC_FORM_WIDE;
    }
    hipLaunchKernelGGL((k_accumulate_tiled<SPAN, kBlock, SUPPORT>), dim3(a.tiles), dim3(kBlock), 0, a.st, a.ps, a.fp, a.target, a.passSeeds, a.tileList, a.argZero);
    return SUPPORT ? ACC_FORM_SUPPORT_TILED : ACC_FORM_TILED;
}

// The accumulate launch itself, for a render and for tinsel_hip_selftest_accumulate alike: `choice` is tinsel_hip_tuning::accumulate;
// shardTiles >= 0: a shard's launch, that many blocks, those of `tileList`; < 0: a block for every tile of the frame; allowSupport = false
// keeps the full window whatever the filter (the selftest's other arm).  Returns the form it ran.
int launch_accumulate_kernels(int numCUs, int choice, bool allowSupport, const uint32_t* passSeeds, const int* tileList, int shardTiles, hipStream_t st,
                              const FrameParams& fp, float4* rad, float4* target)
{
    const PathState ps = { rad };
    if (!accumulate_tiled_fits(fp))
    {
        hipLaunchKernelGGL(k_accumulate, dim3((unsigned)(((size_t)fp.width*fp.height + kBlock - 1)/kBlock)), dim3(kBlock), 0, st, ps, fp, target, passSeeds);
        return ACC_FORM_UNTILED;
    }
    const int tiles = shardTiles >= 0 ? shardTiles : ((fp.width + kAccTile - 1)/kAccTile)*((fp.height + kAccTile - 1)/kAccTile);
    if (tiles == 0)
        return ACC_FORM_TILED;      // (a shard without a candidate in the frame: nothing to add)
    const int span = 1 + (int)floorf(fp.filterWidth) + (int)ceilf(fp.filterWidth) + 1;     // reachLo + reachHi + 1
    // a block per CU or less: piped; up to a wave per SIMD: wide -- unless the tuning names the kernel
    bool piped = tiles <= numCUs;
    bool wide = tiles <= numCUs*4;
    if (choice != TINSEL_ACCUMULATE_AUTO && choice != TINSEL_ACCUMULATE_FULL_WINDOW)
    {
        piped = choice == TINSEL_ACCUMULATE_PIPED;
        wide = choice == TINSEL_ACCUMULATE_WIDE;
    }
    // the support form where the filter allows it (accumulate_support_rule), unless the tuning asks for the full window
    float argZero = 0.0f;
    const bool support = accumulate_support_rule(fp.filterType, fp.filterWidth, fp.filterFalloff, fp.filterOffset, &argZero) &&
                         allowSupport && choice != TINSEL_ACCUMULATE_FULL_WINDOW;
    const AccLaunch a = { passSeeds, tileList, tiles, st, ps, fp, target, support ? argZero : 0.0f };
    if (span == 3)
        return support ? launch_accumulate_span<3, true>(a, piped, wide) : launch_accumulate_span<3, false>(a, piped, wide);
    if (span == 4)
        return support ? launch_accumulate_span<4, true>(a, piped, wide) : launch_accumulate_span<4, false>(a, piped, wide);
    hipLaunchKernelGGL((k_accumulate_tiled<0>), dim3(tiles), dim3(kBlock), 0, st, ps, fp, target, passSeeds, tileList, 0.0f);     // (widths beyond 1: the window's bounds at run time)
    return ACC_FORM_TILED;
}

// The accumulate stage of a traced batch: adds the batch passes [fp.accBegin, fp.accEnd), their radiance at `rad`, to `target`.
// passSeeds: the seed table fp.passBase indexes -- the render call's (null), or a table of the caller's own (feature buffers)
int launch_accumulate(tinsel_hip* r, hipStream_t st, const FrameParams& fp, float4* rad, float4* target, const uint32_t* passSeeds = nullptr)
{
    ScopedTimer t(r, KN_ACCUMULATE, st);
    const bool listed = fp.shardWorld > 1 && accumulate_tiled_fits(fp);         // a shard's launch: the tiles that have candidates of its own
    if (listed && accumulate_tile_list(r, fp))
        return -1;
    launch_accumulate_kernels(r->numCUs, r->tune.accumulate, true, passSeeds ? passSeeds : r->passSeeds, listed ? r->accTilesDev.get() : nullptr, listed ? r->accTilesCount : -1, st, fp,
                              rad, target);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The batch's regions in lane L: at most `grid` region groups (cut_regions, bounded by the lane's arrays) into a.ss; on return *grid is the
// number of groups.  The lane keeps the cut and the batch's paths for tinsel_hip_queue_counts.
int cut_batch(const BatchPlan& p, tinsel_hip::DenseLane& L, LaunchArgs& a, size_t slots, int* grid)
{
    RegionSpec s = p.regions;
    s.maxRegions = L.splitMaxRegions;
    s.capacity = L.splitCap;
    RegionCut c;
    if (!cut_regions(s, slots, *grid, c))
        return fail("render: path buffers too small for this batch");
    a.ss.numRegions = c.numRegions;
    a.ss.regionLen = c.regionLen;
    a.ss.bigRegions = c.bigRegions;
    a.ss.shortLen = c.shortLen;
    L.regions = c.numRegions;
    L.paths = (uint32_t)slots;
    *grid = c.grid();
    return 0;
}

// the timer a generation kernel's launch is reported under (tinsel_hip_kernel_times)
int generate_timer(int generate)
{
    switch (generate)
    {
    case PK_GENERATE_RAYS: return KN_GENERATE_RAYS;
    case PK_GENERATE_GATHER: return KN_GENERATE_GATHER;
    default: return KN_GENERATE;
    }
}

// The split and paired pipelines' batch: cut into regions in lane L and its paths generated.  On return *grid is the launches' grid.
// (k_seg_prefix stages one count per region in LDS, (sharedMemLimit - 1024)/4 of them at most: where a walk list is built the grid is
// clamped to what fits)
int cut_and_generate(tinsel_hip* r, const BatchPlan& p, tinsel_hip::DenseLane& L, hipStream_t st, LaunchArgs& a, size_t slots, int* grid)
{
    *grid = streaming_grid(p.regions, slots);
    if (p.workList)
        *grid = std::max(1, std::min(*grid, (int)(seg_prefix_max_regions(r)/(kBlock/kWave))));
    if (cut_batch(p, L, a, slots, grid))
        return -1;
    // (the plan says which paths: the camera's, a radiance query's -- k_generate_rays reads a.radiance and no camera --, a gather
    // query's -- k_generate_gather reads a.gather --, a views call's -- k_generate_views reads a.views, a.fp and its own seed table -- or a
    // sample map's: k_generate_samples reads a.samples, a.cam, a.fp and its own seed table)
    ScopedTimer t(r, generate_timer(p.generate), st);
    a.grid = *grid;
    a.variant = p.generate;
    a.ldsBytes = 0;
    return launch_path(r, a, st);
}

// region groups, longest first (k_region_order, tn_kernels.h), by the live entries of the regions' fronts and backs
void order_regions(tinsel_hip* r, hipStream_t st, const LaunchArgs& a, const uint32_t* front, const uint32_t* back, uint32_t* out)
{
    ScopedTimer t(r, KN_SEG, st);
    hipLaunchKernelGGL(k_region_order, dim3(1), dim3(kOrderBlock), 0, st, front, back, a.ss.numRegions, out);
}

// the fused pipeline: ONE launch takes every region through all the bounces (k_bounce, tn_kernels.h)
int trace_fused(tinsel_hip* r, const BatchPlan& p, tinsel_hip::DenseLane& L, hipStream_t st, LaunchArgs& a, size_t slots)
{
    int grid = streaming_grid(p.regions, slots);
    if (cut_batch(p, L, a, slots, &grid))
        return -1;
    a.grid = grid;
    // (the shading pools and the waves per SIMD were planned before the batch was cut: plan_bounce)
    if (p.pools)
    {
        a.fp.repack = 1;
        a.ldsBytes += (uint32_t)(kPoolWords*sizeof(uint32_t));
    }
    // bounces > 0: a workgroup's four regions as ONE stream dealt to its waves -- where a round is long (three or more shadow rays)
    // and where the regions are short (a small batch: the ragged last round of every region and bounce weighs more)
    {
        const int shareLen = 512;       // cornell 256^2 x 16 passes (regions of 384): 2258 -> 2311 Msamples/s; 1024^2 x 20 (regions of 2048) +0.3 %
        a.fp.share = r->tune.bounce_share >= 0 ? (r->tune.bounce_share != 0) : (r->neePerPath >= 3 || (int)a.ss.regionLen <= shareLen);
    }
    // (Workgroup b takes region group b: a golden-section step, which k_walk's static ranges need, loses here -- the dispatcher already
    // hands workgroups out dynamically: veach 1970 -> 1904 Msamples/s, features 898 -> 880, cornell 2999 -> 2979.  The per-bounce launches
    // of rounds 1-2, regions longest first, went in round 5.)
    a.bounce = 0;
    a.bounceEnd = a.fp.maxDepth;
    a.order = nullptr;
    a.variant = a.fp.share ? p.bounceShared : p.bounce;
    r->lastBounceKind = a.variant == PK_BOUNCE_FIT_CLOSED ? kBounceFitClosed :
                        a.variant == PK_BOUNCE_FIT_DEFERRED ? kBounceFitDeferred :
                        (a.variant == PK_BOUNCE_COUNT_LDS || a.variant == PK_BOUNCE_COUNT) ? kBounceCount : kBounceGeneral;
    r->lastBounceFeatures = p.bounceFeatures | (a.fp.share ? kFeatShare : 0u);
    ScopedTimer t(r, KN_BOUNCE, st);
    // a baked instance of the closed FIT kernel, where one is installed for exactly the scene level in force (tn_host_bake.h)
    if (a.variant == PK_BOUNCE_FIT_CLOSED && baked_serves(r, a))
        return launch_baked(r, a, st);
    return launch_path(r, a, st);
}

// the paired pipeline: ONE k_walk and ONE streaming kernel per bounce (tn_paired.h): walk { shadow rays of bounce b - 1, extension rays of bounce b }, then k_step(b)
int trace_paired(tinsel_hip* r, const BatchPlan& p, tinsel_hip::DenseLane& L, hipStream_t st, LaunchArgs& a, size_t slots)
{
    int grid = 0;
    if (cut_and_generate(r, p, L, st, a, slots, &grid))
        return -1;
    const size_t W = a.ss.numRegions;
    const int K = r->neePerPath, maxDepth = a.fp.maxDepth;
    // (the step after the last bounce only resolves the last bounce's light samples: nothing to do without lights)
    const int steps = maxDepth + (K > 0 ? 1 : 0);
    for (int bounce = 0; bounce < steps; ++bounce)
    {
        a.bounce = bounce;
        a.order = nullptr;
        if (p.walk)
        {
            a.grid = grid;
            const bool first = bounce == 0, last = bounce >= maxDepth;
            if (launch_walk(r, p, L, st, a, slots, L.ss.segFront + (size_t)bounce*W, /*shadowRays*/ !first && K > 0, /*mixed*/ !first && !last && K > 0))
                return -1;
        }
        // k_step's region groups longest first (k_region_order) where paths are deep: by bounce 6 most regions are nearly empty and the few
        // full ones should not start last -- transmission.tin (depth 16) k_step 13.45 -> 11.81 ms, 1329 -> 1396 Msamples/s; at depth 4 the sort's
        // launch costs what it saves (the 524k-triangle config 2562 / 2555: profiles/r06_r_ab_step_order.md)
        if (bounce > 0 && maxDepth >= 6 && grid > r->numCUs*2)
        {
            order_regions(r, st, a, L.ss.segFront + (size_t)bounce*W, L.ss.segBack + (size_t)bounce*W, L.regionOrder);
            a.order = L.regionOrder;
        }
        ScopedTimer t(r, KN_STEP, st);
        a.grid = grid;
        a.variant = p.step;
        a.ldsBytes = p.ldsTrace;
        a.stackEntries = p.stackScan;
        if (launch_path(r, a, st))
            return -1;
    }
    return 0;
}

// the split pipeline: per bounce k_walk / k_swalk, k_extend, k_lights, k_walk / k_swalk or k_shadow, k_shade
int trace_split(tinsel_hip* r, const BatchPlan& p, tinsel_hip::DenseLane& L, hipStream_t st, LaunchArgs& a, size_t slots)
{
    int grid = 0;
    if (cut_and_generate(r, p, L, st, a, slots, &grid))
        return -1;
    const size_t W = a.ss.numRegions;
    // (the trace kernels stride over the regions: one block per four regions like the others)
    const bool ordered = !p.walk && grid > r->numCUs*2;
    for (int bounce = 0; bounce < a.fp.maxDepth; ++bounce)
    {
        a.bounce = bounce;
        // longest regions first (k_region_order, tn_kernels.h): the paths' order serves k_extend, k_lights and k_shade,
        // the shadow-ray bundles' order k_shadow; bounce 0's regions are all full
        a.order = nullptr;
        if (ordered && bounce > 0)
        {
            order_regions(r, st, a, L.ss.segFront + (size_t)bounce*W, L.ss.segBack + (size_t)bounce*W, L.regionOrder);
            a.order = L.regionOrder;
        }
        const uint32_t* const pathOrder = a.order;
        a.grid = grid;
        if (p.walk && launch_walk(r, p, L, st, a, slots, L.ss.segFront + (size_t)bounce*W, false))
            return -1;
        if (p.sceneWalk)
        {
            if (launch_swalk(r, p, L, st, a, slots, L.ss.segFront + (size_t)bounce*W, L.ss.segBack + (size_t)bounce*W, false))
                return -1;
        }
        else
        {
            ScopedTimer t(r, KN_EXTEND, st);
            a.variant = p.extend;
            a.ldsBytes = p.ldsTrace;
            a.stackEntries = p.stackScan;
            if (launch_path(r, a, st))
                return -1;
        }
        if (r->neePerPath > 0)
        {
            if (p.lights != PK_NONE)
            {
                ScopedTimer t(r, KN_LIGHTS, st);
                a.variant = p.lights;
                a.ldsBytes = p.ldsLights;
                if (launch_path(r, a, st))
                    return -1;
            }
            if (p.walk && launch_walk(r, p, L, st, a, slots, L.ss.neeFront + (size_t)bounce*W, true))
                return -1;
            if (p.sceneWalk)
            {
                if (launch_swalk(r, p, L, st, a, slots, L.ss.neeFront + (size_t)bounce*W, L.ss.neeBack + (size_t)bounce*W, true))
                    return -1;
            }
            else
            {
                if (ordered && bounce > 0)
                {
                    order_regions(r, st, a, L.ss.neeFront + (size_t)bounce*W, L.ss.neeBack + (size_t)bounce*W, L.regionOrderNee);
                    a.order = L.regionOrderNee;
                }
                ScopedTimer t(r, KN_SHADOW, st);
                a.variant = p.shadow;
                a.ldsBytes = p.ldsTrace;
                a.stackEntries = p.stackScan;
                if (launch_path(r, a, st))
                    return -1;
                a.order = pathOrder;
            }
        }
        {
            ScopedTimer t(r, KN_SHADE, st);
            LaunchArgs s = a;
            s.variant = p.shade;
            s.ldsBytes = p.ldsShade;
            s.stackEntries = p.stackScan;
            s.scene.arenaLdsBytes = p.arenaLdsShade;
            if (launch_path(r, s, st))
                return -1;
        }
    }
    return 0;
}

// The slots of a batch of passes fp.passBase .. + fp.numPasses: fills fp's shard numbering, slot count and per-batch settings.
// Returns the batch's slot count, 0 if it does not fit the 32-bit slot index.
size_t batch_frame(const tinsel_hip* r, FrameParams& fp)
{
    // path slots of this shard per pass and per batch (slot_pixel / slot_of, tn_kernels.h): rank-local numbering
    const size_t perPass = slots_per_pass(r, fp.width, fp.height, &fp.shardTilesX, &fp.shardOwnedTiles);
    const size_t slots = perPass*(size_t)fp.numPasses;
    if (slots >= (size_t)0xffffffffu)
        return 0;
    fp.shardPerPass = (uint32_t)perPass;
    {
        auto magic = [](uint32_t d) { return 0xffffffffu/std::max(1u, d); };      // (tn_kernels.h div_magic)
        fp.perPassM = magic(fp.shardPerPass);
        fp.tileSqM = magic((uint32_t)fp.shardTile*(uint32_t)fp.shardTile);
        fp.tileM = magic((uint32_t)fp.shardTile);
        fp.tilesXM = magic((uint32_t)fp.shardTilesX);
    }
    fp.genCount = (uint32_t)slots;
    fp.accBegin = 0;
    fp.accEnd = fp.numPasses;
    fp.rrStart = r->rrStart;
    fp.repack = 0;
    fp.share = 0;
    return slots;
}

// The paths of a batch that the camera does not produce, by the generation kernel that makes them: exactly one is set
struct CallerPaths
{
    const RadianceJob* rays = nullptr;      // a radiance query's records (k_generate_rays, tn_host_radiance.h)
    const GatherJob* gather = nullptr;      // a gather query's points (k_generate_gather, tn_host_gather.h)
    const ViewsJob* views = nullptr;        // a views call's cameras (k_generate_views, tn_host_views.h)
    const SamplesJob* samples = nullptr;    // a sample map's offsets, beside the camera (k_generate_samples, tn_host_samples.h)
    int generate() const { return rays ? PK_GENERATE_RAYS : gather ? PK_GENERATE_GATHER : views ? PK_GENERATE_VIEWS : samples ? PK_GENERATE_SAMPLES : PK_NONE; }
};

// What a side call over the camera's own paths replaces of a render's batch (light groups): the seed table k_generate reads, the statistics
// the kernels count into, the planes k_shade_groups deposits into or k_shade_depths writes (depth planes).  Null / zero: the renderer's own.
struct TraceOverrides
{
    const uint32_t* passSeeds = nullptr;
    unsigned long long* stats = nullptr;
    GroupState groups = { nullptr, nullptr, -1, 0u };
    DepthState depths = { nullptr, 0ull, 0u };
};

// The launches of one batch of `slots` paths in lane L, by the plan's pipeline; a finished path's radiance goes to rad[its slot].  The paths
// are the camera's (`cam`, fp's passes), or the caller's (`starts`: a radiance or a gather query, a views call or a sample map -- the split or the paired
// pipeline behind k_generate_rays / k_generate_gather / k_generate_views / k_generate_samples, p.generate; the fused kernel and k_mega generate the camera's paths themselves).
int trace_batch(tinsel_hip* r, const BatchPlan& p, tinsel_hip::DenseLane& L, hipStream_t st, const CameraParams* cam, const FrameParams& fp, float4* rad,
                size_t slots, const CallerPaths* starts = nullptr, const TraceOverrides* over = nullptr)
{
    if (starts && (p.generate != starts->generate() || (p.pipeline != TINSEL_PIPELINE_WAVEFRONT_SPLIT && p.pipeline != TINSEL_PIPELINE_WAVEFRONT_PAIRED)))
        return fail("trace_batch: caller-started paths run the split or the paired pipeline");
    r->lastPipeline = p.pipeline;

    // what every launch of the batch shares
    LaunchArgs a = launch_base(r);
    a.ps.rad = rad;
    a.ctl = r->ctl;
    if (cam)
        a.cam = *cam;
    if (starts && starts->rays)
        a.radiance = *starts->rays;
    if (starts && starts->gather)
        a.gather = *starts->gather;
    if (starts && starts->views)
        a.views = *starts->views;
    if (starts && starts->samples)
        a.samples = *starts->samples;
    a.fp = fp;
    a.passSeeds = r->passSeeds;
    if (over)
    {
        a.passSeeds = over->passSeeds ? over->passSeeds : a.passSeeds;
        a.ctl.stats = over->stats ? over->stats : a.ctl.stats;
        a.groups = over->groups;
        a.depths = over->depths;
    }
    a.walkRec = p.walk ? L.walkRec : nullptr;
    a.walkPrims = (uint32_t)r->walkPrims.count;
    a.bins = r->binPrims;
    if (p.pipeline == TINSEL_PIPELINE_MEGAKERNEL)
    {
        ScopedTimer t(r, KN_MEGA, st);
        a.grid = (int)std::max<size_t>(1, (slots + kBlock - 1)/kBlock);
        a.variant = p.mega;
        if (launch_path(r, a, st))
            return -1;
    }
    else
    {
        a.ss = L.ss;
        a.ss.radOut = rad;
        const int rc = p.pipeline == TINSEL_PIPELINE_WAVEFRONT ? trace_fused(r, p, L, st, a, slots) :
                       p.pipeline == TINSEL_PIPELINE_WAVEFRONT_PAIRED ? trace_paired(r, p, L, st, a, slots) : trace_split(r, p, L, st, a, slots);
        if (rc)
            return -1;
    }
    r->lastFp = fp;
    return 0;
}

// One batch -- or one overlapped chunk -- of passes fp.passBase .. + fp.numPasses, traced in lane L; the paths' radiance goes to rad[0, slots)
int render_batch(tinsel_hip* r, const BatchPlan& p, tinsel_hip::DenseLane& L, hipStream_t st, const CameraParams& cam, FrameParams fp, float4* rad,
                 bool accumulate = true)
{
    const size_t slots = batch_frame(r, fp);
    if (!slots)
        return fail("render: batch too large");
    if (trace_batch(r, p, L, st, &cam, fp, rad, slots))
        return -1;
    if (!accumulate)
        return 0;
    return launch_accumulate(r, st, fp, rad, r->accum);
}

// The path buffers (ensure_batch) have one user at a time.  Renders order themselves by their stream, and what look-ahead leaves in flight is
// waited for by whoever comes next (lookahead_cancel) -- but the device entry of a radiance query neither waits nor cancels, on a stream of the
// caller's.  So whoever leaves the buffers on a stream the next user cannot know records the fence behind its last launch, and every user
// makes its stream wait for a fence recorded elsewhere before its first.
int batch_fence_wait(tinsel_hip* r, hipStream_t st)
{
    if (r->batchFencePending && r->batchFenceStream != st)
        HIP_TRY(hipStreamWaitEvent(st, r->batchFence, 0));
    return 0;
}

int batch_fence_signal(tinsel_hip* r, hipStream_t st)
{
    if (r->batchFence.create())
        return -1;
    HIP_TRY(hipEventRecord(r->batchFence, st));
    r->batchFenceStream = st;
    r->batchFencePending = true;
    return 0;
}

// st waits, on the device, for what the renderer's own streams hold -- the default one and the look-ahead's (the queryFork events)
int own_streams_wait(tinsel_hip* r, hipStream_t st)
{
    const hipStream_t own[2] = { nullptr, (hipStream_t)r->workStream };
    for (int k = 0; k < 2; ++k)
    {
        if (own[k] == st || (k == 1 && !own[k]))
            continue;
        if (r->queryFork[k].create())
            return -1;
        HIP_TRY(hipEventRecord(r->queryFork[k], own[k]));
        HIP_TRY(hipStreamWaitEvent(st, r->queryFork[k], 0));
    }
    return 0;
}

// The batches of a query: `n` items (a radiance query's paths, a gather query's points) of `pathsEach` paths each, perBatch items at a time in
// the renderer's path buffers, one batch after the other on st; batch(plan, fp, done, m) enqueues the items [done, done + m) with trace_batch
// and what follows it.  Ordered against the buffers' other users by events, both ways and without a host wait: st waits for what the renderer
// has in flight (the default stream's, the look-ahead's, a render or a query on a caller's stream: batch_fence_wait and the fork below),
// nothing of it is discarded, and the fence recorded behind the last launch is what the next user waits for.
template <class Batch>
int trace_caller_batches(tinsel_hip* r, size_t n, size_t perBatch, size_t pathsEach, int generate, int maxDepth, hipStream_t st, Batch batch)
{
    const BatchPlan plan = plan_batch(r, perBatch*pathsEach, 1, /*mayOverlap*/ false, generate);
    if (ensure_batch(r, plan, maxDepth) || batch_fence_wait(r, st) || own_streams_wait(r, st))
        return -1;

    // no pixel, no pass, no shard: the generation count, the depth and the roulette start are all the kernels behind the generation kernel read
    FrameParams fp;
    memset(&fp, 0, sizeof(fp));
    fp.maxDepth = maxDepth;
    fp.rrStart = r->rrStart;
    fp.numPasses = 1;
    fp.shardWorld = 1;
    for (size_t done = 0; done < n; done += perBatch)
    {
        const size_t m = std::min(perBatch, n - done);
        fp.genCount = (uint32_t)(m*pathsEach);
        r->lastLane = 0;
        if (batch(plan, fp, done, m))
            return -1;
    }
    HIP_TRY(hipGetLastError());
    return batch_fence_signal(r, st);
}

// return finished timing events to the pool (a render call's kernel times cover that call alone)
void release_spans(tinsel_hip* r)
{
    for (TimedSpan& s : r->spans)
    {
        r->eventPool.push_back(std::move(s.start));
        r->eventPool.push_back(std::move(s.stop));
    }
    r->spans.clear();
}

// Random(1) advanced `index` times: from the renderer's generator where it has not gone past `index`, else from the seed
Rng seed_rng_at(const tinsel_hip* r, uint32_t index)
{
    const bool behind = r->seedRngIndex <= index;
    Rng g = behind ? r->seedRng : Rng::seeded(1u);
    for (uint32_t at = behind ? r->seedRngIndex : 0; at < index; ++at)
        (void)g.rand();
    return g;
}

// The frame of a render call: size, depth, shard, filter (the batch fields: batch_frame)
FrameParams frame_params(const tinsel_hip* r, const tinsel_options* options)
{
    FrameParams fp;
    fp.width = options->width;
    fp.height = options->height;
    fp.npixM = 0xffffffffu/(uint32_t)std::max(1, options->width*options->height);
    fp.widthM = 0xffffffffu/(uint32_t)std::max(1, options->width);
    fp.maxDepth = options->max_depth;
    fp.shardRank = r->shardRank;
    fp.shardWorld = r->shardWorld;
    fp.shardTile = r->shardTile;
    fp.filterType = options->filter.type;
    fp.filterWidth = options->filter.width;
    fp.filterFalloff = options->filter.falloff;
    fp.filterOffset = options->filter.offset;
    fp.clampLen = options->clamp;
    fp.passBase = 0;
    fp.numPasses = 1;
    return fp;
}

// traceOnly: the passes must fit ONE batch; their paths are traced (radiance left in ps.rad, r->lastFp set) but not
// accumulated -- the caller adds them pass range by pass range (launch_accumulate) into buffers of its choice (look-ahead).
int render_impl(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options, int passes, hipStream_t st, bool traceOnly = false)
{
    if (!r || !camera || !options)
        return fail("render: null argument");
    if (!r->accum || options->width != r->width || options->height != r->height)
        return fail("render: options.width/height do not match the last tinsel_hip_init");
    if (passes < 1)
        return fail("render: passes must be >= 1");
    if (r->sceneDirty)
        return fail("render: a primitive was moved (tinsel_hip_set_primitive_transform): call tinsel_hip_rebuild_scene first");
    HIP_TRY(hipSetDevice(r->device));

    release_spans(r);

    CameraParams cam;
    make_camera(*camera, options->width, options->height, cam);
    FrameParams fp = frame_params(r, options);

    const size_t npix = (size_t)fp.width*fp.height;
    const int gridPix = (int)((npix + kBlock - 1)/kBlock);

    if (options->mode == TINSEL_MODE_NORMALS)
    {
        ScopedTimer t(r, KN_NORMALS, st);
        launch_normals(r, st, gridPix, cam, fp);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    if (options->mode != TINSEL_MODE_PATHTRACE)
        return 0;       // eComplexity is a no-op in the reference too (render.cpp:516-519)
    if (fp.maxDepth < 1)
        return 0;

    // pass seeds: passSeed[s] = (passIndex+s+1)-th output of Random(1).Rand().  The device keeps a TABLE of them, produced there by
    // one thread (k_pass_seeds) from the generator state the host keeps: this call's and the next thousand passes', so that a call
    // launches its path kernels and nothing else (a 256^2 x 16-pass batch is 0.43 ms of kernels: a third launch per call was 1.5 % of it).
    // The table is rewritten only when a call leaves it (every 1024 passes, or a rewind: tinsel_hip_set_pass_index) -- after a
    // device-wide wait, because kernels of another stream (look-ahead) may still read it; a stream other than the one that wrote
    // it waits for the writer's event.
    constexpr size_t kSeedsAhead = 1024;
    const bool covered = r->passSeedsCount > 0 && r->passIndex >= r->passSeedsBase &&
                         (size_t)(r->passIndex - r->passSeedsBase) + (size_t)passes <= r->passSeedsCount;
    if (!covered)
    {
        r->seedRng = seed_rng_at(r, r->passIndex);
        r->seedRngIndex = r->passIndex;
        if (r->passSeedsDev)
            HIP_TRY(hipDeviceSynchronize());
        const size_t want = (size_t)passes + kSeedsAhead;
        r->passSeedsCount = 0;
        if (r->passSeedsDev.grow(want) || r->passSeedsReady.create())
            return -1;
        hipLaunchKernelGGL(k_pass_seeds, dim3(1), dim3(1), 0, st, r->seedRng.s1, r->seedRng.s2, (int)want, r->passSeedsDev.get());
        HIP_TRY(hipEventRecord(r->passSeedsReady, st));
        r->passSeedsBase = r->passIndex;
        r->passSeedsCount = want;
        r->passSeedsStream = st;
    }
    else if (st != r->passSeedsStream)
        HIP_TRY(hipStreamWaitEvent(st, r->passSeedsReady, 0));
    r->passSeeds = r->passSeedsDev.get() + (r->passIndex - r->passSeedsBase);

    const size_t perPass = slots_per_pass(r, fp.width, fp.height);
    const int perBatch = passes_per_batch(batch_slots(r), perPass, passes);

    const BatchPlan plan = plan_batch(r, perPass, perBatch, !traceOnly);
    if (ensure_batch(r, plan, fp.maxDepth) || batch_fence_wait(r, st))
        return -1;

    if (traceOnly && perBatch < passes)
        return fail("render: look-ahead batch does not fit");
    if (plan.lanes == 2 && !r->laneSync.stream)
    {
        tinsel_hip::LaneSync sync;
        if (sync.create())
            return -1;
        r->laneSync = std::move(sync);
    }
    const tinsel_hip::LaneSync& sync = r->laneSync;
    for (int done = 0; done < passes; done += perBatch)
    {
        const int n = std::min(perBatch, passes - done);
        // (the test hooks: tinsel_hip_read_batch_radiance reads the whole batch, tinsel_hip_queue_counts the lane of the chunk traced last)
        r->lastBatchSlots = perPass*(size_t)n;
        if (plan.lanes == 1 || n < 2)
        {
            fp.passBase = done;
            fp.numPasses = n;
            r->lastLane = 0;
            if (render_batch(r, plan, r->lane[0], st, cam, fp, r->ps.rad, !traceOnly))
                return -1;
            continue;
        }
        // the overlapped chunks (plan_batch): chunk c in lane c on its own stream, its radiance at its passes' slots
        const int first = std::min(plan.chunkPasses, (n + 1)/2);
        HIP_TRY(hipEventRecord(sync.fork, st));                       // whatever the caller's stream holds comes first
        HIP_TRY(hipStreamWaitEvent(sync.stream, sync.fork, 0));
        int rc = 0;
        for (int c = 0; c < 2 && !rc; ++c)
        {
            hipStream_t s = c ? sync.stream : st;
            float4* const rad = r->ps.rad + (size_t)(c ? first : 0)*perPass;
            fp.passBase = done + (c ? first : 0);
            fp.numPasses = c ? n - first : first;
            r->lastLane = c;
            rc = render_batch(r, plan, r->lane[c], s, cam, fp, rad, false);
            if (!rc && c)
                rc = hipStreamWaitEvent(s, sync.accDone, 0) == hipSuccess ? 0 : fail("render: hipStreamWaitEvent");
            if (!rc)
                rc = launch_accumulate(r, s, r->lastFp, rad, r->accum);
            if (!rc)
                rc = hipEventRecord(c ? sync.join : sync.accDone, s) == hipSuccess ? 0 : fail("render: hipEventRecord");
        }
        if (!rc)
            rc = hipStreamWaitEvent(st, sync.join, 0) == hipSuccess ? 0 : fail("render: hipStreamWaitEvent");
        if (rc)
        {
            // kernels already enqueued on the second stream still run over the path state and the accumulator: nothing the caller does
            // next (another render on another stream, init, destroy) may overtake them (lookahead_cancel does the same)
            (void)hipStreamSynchronize(sync.stream);
            return -1;
        }
        // (r->lastFp: the whole batch, its radiance at ps.rad)
        r->lastFp.passBase = done;
        r->lastFp.numPasses = n;
        r->lastFp.genCount = (uint32_t)(perPass*(size_t)n);
        r->lastFp.accBegin = 0;
        r->lastFp.accEnd = n;
    }
    r->passIndex += (uint32_t)passes;
    // (the default stream and the look-ahead's are the renderer's own: a query asks those itself, tn_host_radiance.h)
    if (st && st != (hipStream_t)r->workStream && batch_fence_signal(r, st))
        return -1;
    return 0;
}

// The batches of a side pass over the camera's own paths (the cost map, the feature buffers): `passes` passes of frame fp, perBatch whole
// passes at a time, their seeds from the table `seeds` (seeds[s]: pass s of the call).  Per batch the launch record of a one-path-per-lane
// kernel -- the LDS or the plain variant by the scene's residency -- goes to launch(a, fp), which sets its job, times and launches.
template <class Launch>
int side_pass_batches(tinsel_hip* r, const CameraParams& cam, FrameParams fp, int passes, int perBatch, const uint32_t* seeds, int variantLds,
                      int variantPlain, const char* who, Launch launch)
{
    const int variant = residency(r->scene, r->scene.arenaLdsBytes) == RES_LDS ? variantLds : variantPlain;
    for (int done = 0; done < passes; done += perBatch)
    {
        fp.passBase = done;
        fp.numPasses = std::min(perBatch, passes - done);
        const size_t slots = batch_frame(r, fp);
        if (!slots)
            return fail(std::string(who) + ": batch too large");
        LaunchArgs a = launch_base(r);
        a.cam = cam;
        a.fp = fp;
        a.passSeeds = seeds;
        a.grid = (int)((slots + kBlock - 1)/kBlock);
        a.variant = variant;
        if (launch(a, fp))
            return -1;
    }
    return 0;
}

// tinsel_hip_render_cost: k_cost over the passes [passBegin, passBegin + passes), in batches under the megakernel's slot limit.  The seeds
// are the call's own (pass_seed(passBegin + s), the renderer's table and generator are only read) and so is the map: four planes on the
// device, interleaved per pixel on the host.  No path state, accumulator, pass index or statistics are touched.
int render_cost_impl(tinsel_hip* r, const tinsel_camera* camera, const tinsel_options* options, uint32_t passBegin, int passes, uint32_t* out)
{
    if (!r || !camera || !options || !out)
        return fail("render_cost: null argument");
    if (passes < 1)
        return fail("render_cost: passes must be >= 1");
    if (options->mode != TINSEL_MODE_PATHTRACE)
        return fail("render_cost: options.mode must be TINSEL_MODE_PATHTRACE");
    if (!r->accum || options->width != r->width || options->height != r->height)
        return fail("render_cost: options.width/height do not match the last tinsel_hip_init");
    if (r->sceneDirty)
        return fail("render_cost: a primitive was moved (tinsel_hip_set_primitive_transform): call tinsel_hip_rebuild_scene first");
    HIP_TRY(hipSetDevice(r->device));
    release_spans(r);

    const size_t npix = (size_t)r->width*r->height;
    if (options->max_depth < 1)
    {
        memset(out, 0, sizeof(uint32_t)*4*npix);        // no bounce, no ray
        return 0;
    }

    std::vector<uint32_t> seeds((size_t)passes);
    Rng g = seed_rng_at(r, passBegin);
    for (uint32_t& v : seeds)
        v = g.rand();

    DevBuf<uint32_t> seedsDev, costDev;
    if (seedsDev.alloc(seeds.size()) || costDev.alloc(4*npix))
        return -1;
    HIP_TRY(hipMemcpy(seedsDev.get(), seeds.data(), sizeof(uint32_t)*seeds.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(costDev.get(), 0, sizeof(uint32_t)*4*npix));

    CameraParams cam;
    make_camera(*camera, options->width, options->height, cam);
    FrameParams fp = frame_params(r, options);

    const size_t perPass = slots_per_pass(r, fp.width, fp.height);
    // (k_cost runs k_mega's path with counting on -- the scene BVH walk, stacks r->stackNeed deep -- so it takes the megakernel's limit)
    const int perBatch = passes_per_batch(r->maxBatchSlots, perPass, passes);
    const hipStream_t st = nullptr;
    if (side_pass_batches(r, cam, fp, passes, perBatch, seedsDev.get(), PK_COST_LDS, PK_COST, "render_cost", [&](LaunchArgs& a, const FrameParams&) {
            a.cost = costDev.get();
            ScopedTimer t(r, KN_COST, st);
            if (launch_path(r, a, st))
                return -1;
            HIP_TRY(hipGetLastError());
            return 0;
        }))
        return -1;

    std::vector<uint32_t> planes(4*npix);
    HIP_TRY(hipMemcpy(planes.data(), costDev.get(), sizeof(uint32_t)*planes.size(), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < npix; ++k)
        for (int c = 0; c < 4; ++c)
            out[k*4 + c] = planes[(size_t)c*npix + k];
    return 0;
}


} // namespace

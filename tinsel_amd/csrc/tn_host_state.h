// tn_host_state.h -- struct tinsel_hip: everything a renderer owns
// (part of the library's one host translation unit: included by tinsel_hip.hip, in this order, never on its own)
#pragma once

// the defaults of include/tinsel_hip.h's tinsel_hip_tuning: "the library decides" everywhere
inline tinsel_hip_tuning tuning_defaults()
{
    tinsel_hip_tuning t;
    memset(&t, 0, sizeof(t));
    t.struct_bytes = (uint32_t)sizeof(t);
    t.flat_scan = t.lds_scene = t.walk = t.inline_max_tris = t.walk_min_tris = -1;
    t.small_mesh_bytes = t.arena_lds_limit = -1;
    t.batch_paths = 0;
    t.grid_mult = 0;
    t.bounce_share = t.repack = t.tail_split = t.shade_sorted = t.overlap = t.scene_walk = t.swalk_lds = -1;
    t.tail_share = 0.0f;
    t.tail_divide = 4;
    t.accumulate = TINSEL_ACCUMULATE_AUTO;
    t.walk_block = 0;
    t.walk_single = t.walk_lds_stack = t.quads_in_scan = t.bounce_fit = t.plane_pairs = -1;
    t.walk_refill_min = t.walk_leaf_min = t.walk_grid_mult = 0;
    return t;
}

// a caller's struct, possibly shorter than this build's: the fields it has over the defaults
inline tinsel_hip_tuning tuning_from_caller(const tinsel_hip_tuning* in)
{
    tinsel_hip_tuning t = tuning_defaults();
    if (in && in->struct_bytes >= sizeof(uint32_t))
        memcpy(&t, in, std::min<size_t>(in->struct_bytes, sizeof(t)));
    t.struct_bytes = (uint32_t)sizeof(t);
    return t;
}

struct tinsel_hip
{
    int device = 0;
    int numCUs = 256;
    tinsel_hip_tuning tune = tuning_defaults();     // (tinsel_hip_create_tuned / tinsel_hip_set_tuning; nothing is read from the environment)

    DevPool sceneMem;                   // every upload of the scene: the arena, the meshes in HBM, the probe
    DevScene scene;
    int stackNeed = 16;
    int neePerPath = 0;

    // mesh table as uploaded (reference trees) and as it currently is; device-built trees (tn_lbvh.h)
    std::vector<DevMesh> meshesRef, meshesNow;
    // what a refit needs on the host (tinsel_hip_refit_mesh): per mesh the vertex count and the index triples, per
    // primitive its mesh and the endTransform scale of PrimitiveArea
    std::vector<int> meshNumVertices;
    std::vector<std::vector<int32_t>> meshIndices;
    std::vector<int> primMesh;
    std::vector<int32_t> lightPrims;    // primitives with lightSamples > 0
    std::vector<float> primEndScale;
    // ... and what moving a PRIMITIVE needs (tinsel_hip_set_primitive_transform / tinsel_hip_rebuild_scene): the Prim64 records as
    // uploaded, where they and the Moving64 slots (one per primitive) sit in the arena, every mesh's root box in mesh space and its
    // area (PrimitiveBounds, PrimitiveArea), whether a transform changed since the scene BVH was last built
    std::vector<Prim64> primsHost;
    size_t arenaOffPrims = 0, arenaOffMoving = 0, arenaOffMats = 0;
    std::vector<V3> meshRootLo, meshRootHi;
    std::vector<float> meshArea;
    bool sceneDirty = false;
    // ... and to follow a refitted mesh at the SCENE level (its primitives' leaf boxes and their ancestors in the scene BVH):
    // the primitives' start / end transforms, the reference's scene BVH as handed in, where its device form and the leaf boxes
    // sit in the arena
    std::vector<Xform> primStart, primEnd;
    std::vector<tinsel_bvh_node> sceneBvhHost;
    size_t arenaOffNodes = 0, arenaOffBoxes = 0;
    std::vector<int32_t> planeTablePrims;       // the planes DevScene::planeEq holds (their PrimBox says 2: re-marked when the boxes are rewritten)
    bool pairablePlanes = true;                 // false: this scene's fused instances carry no pair code (several arena meshes, none in HBM)
    int planePairs = 0, planeSingles = 0;       // ... of them as opposing pairs / single planes in the scene level in force
    int sceneStackNeed = 1;
    std::string prepRefused;            // non-empty: a kernel whose dynamic-LDS limit the runtime refused to raise (prepare_kernels_once)
    bool sceneEnclosed = false;         // two planes face each other: (practically) no ray leaves the scene (k_bounce's shading pools stay off)
    int bvhMode = TINSEL_BVH_REFERENCE;
    int rrStart = 0;                    // > 0: Russian roulette from this bounce on (opt-in)
    bool anyTransmission = false;       // a material has a transmission lobe (materials never change after create)
    bool anySubsurface = false;         // a material's subsurface is not +0.0f by its bits (the same; scene_slim, tn_host_batch.h)
    int lastBounceKind = -1;            // k_bounce's last launch: its kind (tn_fused.h BounceKind) and the features asked of it (tinsel_hip_bounce_plan)
    uint32_t lastBounceFeatures = 0;
    DevPool lbvhTrees;                  // the device-built mesh trees in force (set_mesh_bvh: one generation)
    // baked instances (tn_host_bake.h): the host's copy of the scene level in force (adopt_scene_level) and of the lights' own Mat128
    // records (create; write_mesh_prim_area follows a refit) -- what the generated header states --, and the installed code object
    std::vector<float> levelPlaneEq;
    std::vector<int32_t> levelPlaneIdx;
    std::vector<PrimBox> levelBoxes;
    std::vector<Mat128> lightMats;      // by light, in lightPrims' order
    struct Baked
    {
        Module module;
        hipFunction_t fn = nullptr;
        std::string key;                // of the text the module was compiled from
        int mode = -1;                  // tinsel_hip_set_bounce_bake: -1 auto, 0 never serve, 1 wanted at any size
        int how = 0;                    // TINSEL_BAKE_COMPILED / _FROM_CACHE (installed), _NO_COMPILER (nothing installed, and why)
        uint32_t ldsLimit = 65536;      // dynamic LDS a launch of fn may ask for
        unsigned long long launches = 0;
    } baked;

    int width = 0, height = 0;
    // The accumulator every kernel and entry point reads: a VIEW.  It is accumOwn's buffer (tinsel_hip_init; look-ahead moves buffers between
    // accumOwn, specFree and the shots), the caller's (tinsel_hip_init_external: accumOwn empty, nothing to free), or for one call the group's
    // reduced frame (tinsel_hip_group_present).
    float4* accum = nullptr;
    DevBuf<float4> accumOwn;

    // sharded renders: accumulate tiles that have candidate paths of this shard (k_accumulate_tiled)
    DevBuf<int> accTilesDev;
    int accTilesCount = 0;
    int accTilesKey[6] = { 0, 0, 0, 0, 0, 0 };     // width, height, rank, world, shard tile, halo reach

    // display stage (tn_display.h): [0] filtered, [1] NLM means, [2] NLM output; sized width*height on first use
    DevBuf<float4> display[3];
    const float4* presented = nullptr;

    // path batch buffers
    size_t batchSlots = 0;
    int batchNee = -1;
    int batchDepth = -1;
    DevPool batchMem;
    PathState ps;
    QueueCtl ctl;
    int batchPipeline = -1;             // the pipeline the current batch buffers were allocated for
    BinPrims binPrims = { 0, { 0, 0, 0, 0, 0, 0, 0 } };
    BinPrims walkPrims = { 0, { 0, 0, 0, 0, 0, 0, 0 } };   // the subset of binPrims whose closest hits k_walk computes (large trees)
    int walkPrimMesh[7] = { 0, 0, 0, 0, 0, 0, 0 };         // DevScene::meshes index of each walked primitive
    // The wavefront pipelines' dense state (SplitState, tn_kernels.h), by lane: lane 1 only where render_impl traces a batch as two
    // overlapped chunks on two streams (plan_batch), each chunk's accumulate behind the other chunk's kernels.  The split pipeline's
    // hit / shadow-ray arrays only when that is the pipeline in force.
    struct DenseLane
    {
        SplitState ss;
        size_t splitCap = 0;                // positions per SplitState array: the batch slots + one wave of padding per region
        uint32_t splitMaxRegions = 0;
        uint32_t* regionOrder = nullptr;    // region groups, longest first (k_region_order): by live paths, by shadow-ray bundles
        uint32_t* regionOrderNee = nullptr;
        uint32_t* walkList = nullptr;       // k_walk's / k_swalk's work list (k_seg_expand) and the prefix of the regions' front counts behind it
        uint32_t* segPrefix = nullptr;
        float4* walkRec = nullptr;          // k_walk's closest-hit records (tn_walk.h); batch-sized
        uint32_t regions = 0, paths = 0;    // of the chunk last traced here: its regions and paths (tinsel_hip_queue_counts)
    } lane[2];
    // k_walk's stack entries beyond the LDS ones (tinsel_hip_tuning::walk_lds_stack), by lane: grown by ensure_walk_overflow, freed with the
    // renderer, not with the batch
    DevBuf<uint32_t> walkOverflow[2];
    int lastLane = 0;                   // the lane of the chunk traced last
    int batchLanes = 1;                 // lanes allocated (1 or 2)
    size_t batchStateSlots = 0;         // path slots each lane holds (batchSlots: what ps.rad holds)
    // the second chunk's stream and the events that order the two chunks: all of them or none (render_impl makes them in a local)
    struct LaneSync
    {
        Stream stream;
        Event fork, join, accDone;
        int create() { return stream.create() || fork.create() || join.create() || accDone.create() ? -1 : 0; }
    } laneSync;
    bool walkEnabled = true;                            // tinsel_hip_tuning::walk == 0: walk meshes inline in k_extend / k_shadow (A/B)
    DevBuf<unsigned long long> walkProf;                // developer-only (-DTN_WALK_PROF builds): section counters of k_walk
    DevBuf<uint2> probeAlias;                           // alias table of the probe (tinsel_hip_set_probe_sampling), built on first use
    int sharedMemLimit = 65536;
    DevBuf<uint32_t> passSeedsDev;      // the table: the seeds of passes [passSeedsBase, passSeedsBase + passSeedsCount)
    size_t passSeedsCount = 0;
    uint32_t passSeedsBase = 0;
    const uint32_t* passSeeds = nullptr;    // the current call's first seed, inside the table
    Event passSeedsReady;                   // recorded behind the launch that wrote the table, on passSeedsStream
    hipStream_t passSeedsStream = nullptr;
    DevBuf<unsigned long long> statsDev;
    // ray queries (tinsel_hip_trace_rays / tinsel_hip_trace_camera): the host entries' chunk buffers, grown on demand, freed with the renderer
    DevBuf<unsigned char> queryRaysDev, queryOutDev;
    // k_query_refill's cursors: a ring of words, one per launch, and per word the event behind the launch that used it last (launch_query)
    static constexpr uint32_t kQueryCursors = 64;
    struct QueryCursors
    {
        DevBuf<uint32_t> words;
        Event done[kQueryCursors];
        bool used[kQueryCursors] = {};
        uint32_t next = 0;
        int create()
        {
            if (words.alloc(kQueryCursors))
                return -1;
            for (Event& e : done)
                if (e.create())
                    return -1;
            return 0;
        }
    };
    std::unique_ptr<QueryCursors> queryCursors;     // made whole by launch_query on first use
    // radiance queries (tinsel_hip_trace_radiance*, tn_host_radiance.h) trace in the path buffers: the event behind their last user on a
    // stream the next user cannot know (batch_fence_signal / batch_fence_wait, tn_host_batch.h), and the events a query records on the
    // renderer's own streams -- [0] the default one, [1] the look-ahead's -- to wait for what they hold
    Event batchFence, queryFork[2];
    hipStream_t batchFenceStream = nullptr;
    bool batchFencePending = false;
    // gather queries (tinsel_hip_gather_radiance*, tn_host_gather.h): the radiance of a batch's paths by slot, which k_gather_reduce reads;
    // grown on demand, and the host entry's tinsel_path_start records where the caller asks for them
    DevBuf<unsigned char> gatherRad, gatherStartsDev;
    // feature buffers (tinsel_hip_render_features*, tn_host_features.h): k_features' records of a batch (16 bytes per requested plane and
    // path slot), the call's own seed table, the host entry's planes -- grown on demand, freed with the renderer -- and the event behind the
    // last call's last launch, which a call on another stream waits for before it writes them
    DevBuf<unsigned char> featRec, featOut;
    DevBuf<uint32_t> featSeeds;
    Event featFence;
    hipStream_t featFenceStream = nullptr;
    bool featFencePending = false;
    // ID mattes (tinsel_hip_render_id_mattes*, tn_host_ids.h): k_ids' records of a batch (4 bytes per path slot), the per-pixel lists the
    // batches of a call carry (72 bytes per pixel: eight ids, eight weights, residual, total -- planar), the call's own seed table, the host
    // entry's ranked planes -- grown on demand, freed with the renderer -- and the event behind the last call's last launch, which a call on
    // another stream waits for before it writes them
    DevBuf<unsigned char> idsRec, idsState, idsOut;
    DevBuf<uint32_t> idsSeeds;
    Event idsFence;
    hipStream_t idsFenceStream = nullptr;
    bool idsFencePending = false;
    // light groups (tinsel_hip_render_light_groups*, tn_host_light_groups.h): the planes' records of a batch (16 bytes per group and path
    // slot), the call's own seed table, the primitives' groups (one byte each; groupsTableHost: what was uploaded last), the statistics its
    // kernels count into (never read), the host entry's planes -- grown on demand, freed with the renderer -- and the event behind the last
    // call's last launch, which a call on another stream waits for before it writes them
    DevBuf<unsigned char> groupsRec, groupsOut;
    DevBuf<uint32_t> groupsSeeds;
    DevBuf<int8_t> groupsTable;
    std::vector<int8_t> groupsTableHost;
    DevBuf<unsigned long long> groupsStats;
    Event groupsFence;
    hipStream_t groupsFenceStream = nullptr;
    bool groupsFencePending = false;
    // depth planes (tinsel_hip_render_depth_planes*, tn_host_depth_planes.h): the planes' records of a batch (16 bytes per plane and path
    // slot), the call's own seed table, the statistics its kernels count into (never read), the host entry's planes -- grown on demand, freed
    // with the renderer -- and the event behind the last call's last launch, which a call on another stream waits for before it writes them
    DevBuf<unsigned char> depthsRec, depthsOut;
    DevBuf<uint32_t> depthsSeeds;
    DevBuf<unsigned long long> depthsStats;
    Event depthsFence;
    hipStream_t depthsFenceStream = nullptr;
    bool depthsFencePending = false;
    // view batches (tinsel_hip_render_views*, tn_host_views.h): the radiance of a batch's paths by slot ([view][pass][pixel]), the cameras'
    // table, the call's own seed table, the statistics its kernels count into (never read), the host entry's planes -- grown on demand,
    // freed with the renderer -- and the event behind the last call's last launch, which a call on another stream waits for before it
    // writes them
    DevBuf<unsigned char> viewsRad, viewsOut;
    DevBuf<ViewCamera> viewsCameras;
    DevBuf<uint32_t> viewsSeeds;
    DevBuf<unsigned long long> viewsStats;
    Event viewsFence;
    hipStream_t viewsFenceStream = nullptr;
    bool viewsFencePending = false;
    // sample maps (tinsel_hip_render_sample_map*, tn_host_samples.h): the radiance of a batch's paths by compact slot, the batch's offset
    // table (W*H + 1 entries, uploaded per batch), the call's own seed table, the statistics its kernels count into (never read), the host
    // entry's plane -- grown on demand, freed with the renderer -- and the event behind the last call's last launch, which a call on
    // another stream waits for before it writes them
    DevBuf<unsigned char> samplesRad, samplesOut;
    DevBuf<uint32_t> samplesOff, samplesSeeds;
    DevBuf<unsigned long long> samplesStats;
    Event samplesFence;
    hipStream_t samplesFenceStream = nullptr;
    bool samplesFencePending = false;
    // denoise stage (tinsel_hip_denoise*, tn_host_denoise.h): [0] the filter's colour input U, [1] its patch means, [2] (albedo, depth),
    // [3] the mean normal -- sized to the largest frame denoised -- the host entries' inputs (beauty, planes) and output on the device, and
    // the event behind the last call's last launch, which a call on another stream waits for before it writes them
    DevBuf<float4> denoise[4];
    DevBuf<unsigned char> denoiseIn, denoiseOut;
    Event denoiseFence;
    hipStream_t denoiseFenceStream = nullptr;
    bool denoiseFencePending = false;

    size_t lastBatchSlots = 0;          // paths of the last batch (tinsel_hip_read_batch_radiance)
    int lastPipeline = TINSEL_PIPELINE_WAVEFRONT;   // of the last batch (queue_counts)
    size_t maxBatchSlots = 8u << 20;
    bool batchSlotsExplicit = false;     // set by tinsel_hip_tuning::batch_paths / tinsel_hip_set_batch_paths
    int pipeline = TINSEL_PIPELINE_AUTO;
    int arith = TINSEL_ARITH_EXACT;     // which build of the path kernels runs (tinsel_hip_set_arithmetic)
    bool pathKernelsPrepared = false;
    int segPrefixLds = 0;               // dynamic LDS k_seg_prefix may ask for (prepare_path_kernels): one count per region
    bool countDetail = false;

    uint32_t passIndex = 0;
    Rng seedRng = Rng::seeded(1u);      // Random(1) advanced seedRngIndex times: the generator of the pass seeds
    uint32_t seedRngIndex = 0;
    int shardRank = 0, shardWorld = 1, shardTile = 32;

    // look-ahead (tinsel_hip_set_lookahead): the NEXT call's passes are traced speculatively into accumSpec while this
    // call's running sum travels to the host
    int lookahead = 0;                  // 0 off, 1 on, 2 on + the caller's output array page-locked in place (TINSEL_LOOKAHEAD_PIN_OUTPUT)
    FrameParams lastFp;                 // of the most recent batch (its paths' radiance is still in ps.rad)
    struct SpecShot { DevBuf<float4> buf; Event ready; };
    std::vector<DevBuf<float4>> specFree;      // accumulator-sized buffers not in use
    std::deque<SpecShot> specQueue;     // specQueue[j] = accum + the passes of the next j+1 calls, in flight or finished on workStream
    uint32_t specNextPass = 0;          // pass index the next speculated call starts at
    tinsel_camera specCamera;
    tinsel_options specOptions;
    int specPasses = 0;
    int lookaheadDepth = 0;             // calls per speculated batch; 0 = chosen from the batch capacity 
    Stream workStream, copyStream;      // both or neither (lookahead_streams)
    PinnedOutput pinned;                // the caller's output array, page-locked in place for the D2H DMA

    // process-per-GPU arm of the reduce (tinsel_hip_comm_*, tn_host_group.h): this rank's RCCL communicator
    void* comm = nullptr;               // ncclComm_t
    int commRank = 0, commWorld = 0;

    bool timing = false;
    std::vector<TimedSpan> spans;
    std::vector<Event> eventPool;       // timing events not in use: nothing is created or destroyed per launch once the pool is warm
    double gpuSeconds = 0.0;
};

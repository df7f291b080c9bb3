// tn_host_query.h -- ray queries on the resident scene: the plan of k_query's launch, the launch, the host entries' staging buffers
// (part of the library's one host translation unit: included by tinsel_hip.hip, in this order, never on its own)
#pragma once

namespace {

// rays per chunk of the host entry: 32 MB of rays + 32 MB of records on the device, whatever n is
constexpr size_t kQueryChunk = (size_t)1 << 20;

// rays per launch of tinsel_hip_trace_camera (a 128 MB record buffer the renderer keeps; a 1920 x 1080 frame is one launch)
constexpr size_t kQueryCameraChunk = (size_t)1 << 22;

// k_query's launch for one mode on the scene in force (tn_query.h): the instance by residency -- the whole scene staged (LDS), or generic
// pointers over the bytes scene.arenaLdsBytes says with the other meshes in HBM, as k_normals / k_cost -- workgroups of kBlock, stacks at the
// scene's planned depth, and the ARM, by what was measured on 2^22 incoherent rays (profiles/r07_ray_query.md):
//   k_query          one ray per lane, trace<> as the path kernels run it: closest hits on flat-scan scenes (ajax_standin_96 0.383 ms against
//                    0.423, glass 0.353 against 0.480: the wave-uniform scan beats a divergent walk over a handful of primitives), every
//                    camera frame (coherent rays), occlusion where the whole scene sits in LDS;
//   k_query_refill   persistent workgroups with ray replacement on the scene BVH walk: scenes beyond the flat scan (many_spheres closest
//                    0.358 -> 0.245 ms, occluded 0.150 -> 0.133) and occlusion on flat-scan scenes with meshes in HBM (ajax_standin_96
//                    0.348 -> 0.196 ms: the walk stops at the first hit below tmax, the scan runs every mesh walk to its end).
struct QueryPlan
{
    int variant = PK_NONE;
    int block = kBlock;
    int stackEntries = 0;
    uint32_t arenaLds = 0;          // arena bytes the kernel stages
    uint32_t ldsBytes = 0;
    int persistent = 0;             // > 0: k_query_refill, that many workgroups at most, each taking rays until none is left
    int grid(size_t n) const
    {
        const size_t g = (n + (size_t)block - 1)/(size_t)block;
        return (int)(persistent > 0 ? std::min<size_t>(g, (size_t)persistent) : g);
    }
};

QueryPlan plan_query(const tinsel_hip* r, int mode)
{
    static const int kPlain[3][2] = { { PK_QUERY_CLOSEST, PK_QUERY_CLOSEST_LDS }, { PK_QUERY_OCCLUDED, PK_QUERY_OCCLUDED_LDS },
                                      { PK_QUERY_CAMERA, PK_QUERY_CAMERA_LDS } };
    static const int kRefill[2][2] = { { PK_QUERYR_CLOSEST, PK_QUERYR_CLOSEST_LDS }, { PK_QUERYR_OCCLUDED, PK_QUERYR_OCCLUDED_LDS } };
    const int lds = residency(r->scene, r->scene.arenaLdsBytes) == RES_LDS ? 1 : 0;
    const bool refill = mode != kQueryCamera && (r->scene.flatScan == 0 || (mode == kQueryOccluded && !lds));
    QueryPlan p;
    p.variant = refill ? kRefill[mode][lds] : kPlain[mode][lds];
    p.stackEntries = r->stackNeed;
    p.arenaLds = r->scene.arenaLdsBytes;
    p.ldsBytes = (uint32_t)stack_bytes(r);
    p.persistent = refill ? r->numCUs*TN_WAVES_TRACE : 0;       // (a workgroup is one wave per SIMD: TN_WAVES_TRACE of them fill a CU)
    return p;
}

// enqueues k_query over n rays (device pointers) on st; mode: QueryMode
int launch_query(tinsel_hip* r, int mode, size_t n, const void* rays, void* out, const CameraParams* cam, int width, float time, hipStream_t st,
                 uint32_t first = 0)
{
    const QueryPlan plan = plan_query(r, mode);
    LaunchArgs a = launch_base(r);
    a.scene.arenaLdsBytes = plan.arenaLds;
    if (cam)
        a.cam = *cam;
    a.query.rays = rays;
    a.query.out = out;
    a.query.n = (uint32_t)n;
    a.query.width = width;
    a.query.time = time;
    a.query.first = first;
    hipEvent_t slotDone = nullptr;
    if (plan.persistent > 0)
    {
        // A cursor word of this launch's own, out of a ring: queries on different streams may run side by side (the device entry does not
        // wait), so they cannot share one.  The word is zeroed on THIS stream in front of the kernel; before a slot is used again, this
        // stream waits for the launch that had it last.
        if (!r->queryCursors)
        {
            std::unique_ptr<tinsel_hip::QueryCursors> ring(new tinsel_hip::QueryCursors());
            if (ring->create())
                return -1;
            r->queryCursors = std::move(ring);
        }
        tinsel_hip::QueryCursors& ring = *r->queryCursors;
        const uint32_t slot = ring.next++ % tinsel_hip::kQueryCursors;
        slotDone = ring.done[slot];
        if (ring.used[slot])
            HIP_TRY(hipStreamWaitEvent(st, slotDone, 0));
        ring.used[slot] = true;
        HIP_TRY(hipMemsetAsync(ring.words.get() + slot, 0, sizeof(uint32_t), st));
        a.query.cursor = ring.words.get() + slot;
    }
    a.stackEntries = plan.stackEntries;
    a.ldsBytes = plan.ldsBytes;
    a.grid = plan.grid(n);
    a.variant = plan.variant;
    {
        ScopedTimer t(r, KN_QUERY, st);
        if (launch_path(r, a, st))
            return -1;
    }
    HIP_TRY(hipGetLastError());
    if (slotDone)
        HIP_TRY(hipEventRecord(slotDone, st));
    return 0;
}

int query_ready(tinsel_hip* r, const char* who)
{
    if (r->sceneDirty)
        return fail(std::string(who) + ": a primitive was moved (tinsel_hip_set_primitive_transform): call tinsel_hip_rebuild_scene first");
    HIP_TRY(hipSetDevice(r->device));
    if (r->timing)
        release_spans(r);           // (as a render call: tinsel_hip_kernel_times reports the most recent call's kernels)
    return 0;
}

int query_buffer(DevBuf<unsigned char>& buf, size_t bytes)
{
    if (buf && buf.count() < bytes)
        HIP_TRY(hipDeviceSynchronize());
    return buf.grow(bytes);
}

// The arrays of a device entry: each 16-byte aligned, no two non-empty ones overlapping
struct QueryArray
{
    const void* p;
    size_t bytes;
};

int query_arrays(std::initializer_list<QueryArray> arrays, const char* who)
{
    for (const QueryArray* i = arrays.begin(); i != arrays.end(); ++i)
    {
        const uintptr_t a = (uintptr_t)i->p;
        if (a & 15u)
            return fail(std::string(who) + ": the arrays must be 16-byte aligned");
        for (const QueryArray* j = arrays.begin(); j != i; ++j)
            if (i->bytes && j->bytes && a < (uintptr_t)j->p + j->bytes && (uintptr_t)j->p < a + i->bytes)
                return fail(std::string(who) + ": the arrays overlap");
    }
    return 0;
}

// A host entry's arrays go through staging buffers on the device, `chunk` records at a time: `stride` bytes of record k at host + k*stride
// (host null: no such array)
struct StagedIn
{
    const void* host;
    DevBuf<unsigned char>* dev;
    size_t stride;
};

struct StagedOut
{
    void* host;
    DevBuf<unsigned char>* dev;
    size_t stride;
};

// The host entries' loop over n records: the buffers grown to a chunk, then per chunk [done, done + m) the input uploaded (where there is one),
// run(done, m) -- which enqueues the chunk's work on the null stream, reading and writing the buffers from their starts -- and the outputs
// downloaded (out2 where there is one).  The copies are synchronous.
template <class Run>
int staged_chunks(size_t n, size_t chunk, StagedIn in, StagedOut out, StagedOut out2, Run run)
{
    if (chunk == 0)
        return 0;
    if ((in.host && query_buffer(*in.dev, chunk*in.stride)) || query_buffer(*out.dev, chunk*out.stride) ||
        (out2.host && query_buffer(*out2.dev, chunk*out2.stride)))
        return -1;
    for (size_t done = 0; done < n; done += chunk)
    {
        const size_t m = std::min(chunk, n - done);
        if (in.host)
            HIP_TRY(hipMemcpy(in.dev->get(), (const unsigned char*)in.host + done*in.stride, m*in.stride, hipMemcpyHostToDevice));
        if (run(done, m))
            return -1;
        HIP_TRY(hipMemcpy((unsigned char*)out.host + done*out.stride, out.dev->get(), m*out.stride, hipMemcpyDeviceToHost));
        if (out2.host)
            HIP_TRY(hipMemcpy((unsigned char*)out2.host + done*out2.stride, out2.dev->get(), m*out2.stride, hipMemcpyDeviceToHost));
    }
    return 0;
}

} // namespace

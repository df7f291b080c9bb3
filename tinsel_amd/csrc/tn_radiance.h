// tn_radiance.h -- radiance queries (tinsel_hip_trace_radiance*): k_generate_rays, the split and paired pipelines' generation kernel for
// paths the CALLER starts.  It is k_generate with the camera taken out: a record (tinsel_path_start, 48 bytes) gives the ray, the shutter
// time and the two generator words PathTrace() is entered with, and everything downstream -- k_extend .. k_shade, k_walk, k_step -- reads
// buffer 0 of the dense state as it does after k_generate.  A path's slot is its record's index in the batch, and SplitState::radOut is the
// caller's output array: a finished path writes its radiance there, no gather and no copy.
//
// A lane reads its record as three consecutive 16-byte loads (a wave: 3 KiB contiguous), typed as HBM like k_query's rays (tn_walk.h's
// GlobalF4): the caller's pointer is generic to the compiler, and generic loads are flat ones that wait on both counters.  The rays of
// neighbouring lanes have nothing to do with each other, which costs nothing downstream: positions come from the wave's ballot
// (RegionAppend), so the front of a region is still all rays that enter a walked mesh's box and its back all others.
#pragma once

#include "tn_split.h"

namespace tn {

struct RadianceJob
{
    const void* starts;     // tinsel_path_start[first + count], 16-byte aligned
    uint32_t first;         // the record of the batch's slot 0 (a query of more paths than a batch holds runs as several)
    uint32_t count;         // paths of the batch
};

__global__ __launch_bounds__(kBlock, 4) void k_generate_rays(SplitState ss, QueueCtl q, RadianceJob job, const PrimBox* __restrict__ primBoxes, BinPrims bp)
{
    const uint32_t lane = __lane_id();
    const GlobalF4 starts = as_global(job.starts) + (size_t)job.first*3u;
    uint32_t samples = 0;
    for (uint32_t r = blockIdx.x*(kBlock/kWave) + wave_in_block(); r < ss.numRegions; r += gridDim.x*(kBlock/kWave))
    {
        const uint32_t begin = region_base(ss, r), rLen = region_len(ss, r);
        RegionAppend out = { begin, rLen, 0u, 0u };
        const uint32_t end = (begin + rLen) < job.count ? (begin + rLen) : job.count;
        for (uint32_t i0 = begin; i0 < end; i0 += kWave)
        {
            const uint32_t slot = i0 + lane;
            const bool live = slot < end;
            bool front = true;
            PathRegs p;
            if (live)
            {
                const GlobalF4 rec = starts + (size_t)slot*3u;
                const WalkF4 ro = rec[0], rd = rec[1], rg = rec[2];
                Rng rng;
                rng.s1 = __float_as_uint(rg.x);
                rng.s2 = __float_as_uint(rg.y);
                path_begin(p, V3(ro.x, ro.y, ro.z), V3(rd.x, rd.y, rd.z), ro.w, rng);
                // rays that enter a mesh in HBM in front (k_walk takes those), as k_generate sorts the camera's
                front = bp.count == 0 || ray_enters_big_mesh(primBoxes, bp, p.o, p.d);
                samples++;
            }
            const uint32_t pos = out.push(live, front);
            if (live)
            {
                // ray and RNG only, as k_generate: the rest of a fresh path's state is constant and k_shade knows it (ShadeFetch::issue)
                ss.rayO[0][pos] = make_float4(p.o.x, p.o.y, p.o.z, p.time);
                ss.rayD[0][pos] = make_float4(p.d.x, p.d.y, p.d.z, p.bsdfPdf);
                ss.rngId[0][pos] = make_float4(__uint_as_float(p.rng.s1), __uint_as_float(p.rng.s2), __uint_as_float(slot), __int_as_float(-1));
            }
        }
        if (lane == 0)
        {
            ss.segFront[r] = out.nFront;
            ss.segBack[r] = out.nBack;
        }
    }
    wave_add_stat(q.stats, 1, samples);
}

} // namespace tn

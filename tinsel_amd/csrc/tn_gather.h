// tn_gather.h -- gather queries (tinsel_hip_gather_radiance*): S paths from each of n surface points, one mean radiance per point back.
// k_generate_gather is the third generation kernel beside k_generate (the camera's paths) and k_generate_rays (paths the caller starts),
// a third source of paths for generate_regions (tn_split.h): a point (tinsel_gather_point, 32 bytes: position, shutter time, normal, seed) and a sample index give the path -- generator
// Random(seed + s), two draws, a direction about the normal (BasisFromVector + CosineSampleHemisphere, composed as disney.h:256-258 does:
// U*d.x + V*d.y + N*d.z, summed left to right) or on the sphere (UniformSampleSphere) -- and everything downstream reads buffer 0 of the
// dense state as it does after k_generate.  k_gather_reduce, behind the pipeline, sums a point's S results in ascending s and divides;
// k_gather_sh_reduce (tinsel_hip_gather_sh*) sums them times the SH basis at each path's direction instead.
//
// The slot <-> (point, sample) map inside a batch of P whole points is SAMPLE-major: slot = s*P + point.  A wave of k_generate_gather then
// reads 64 consecutive points (2 KiB contiguous, two 16-byte loads per lane typed as HBM like k_generate_rays' records), and a wave of
// k_gather_reduce, one lane per point, reads 1 KiB contiguous of the batch's radiance per sample; point-major, each of its lanes would
// stride by 16*S bytes.  The map shows nowhere outside: `startsOut`, where asked for, is written at point*S + s, and a point's sum does not
// depend on which batch it fell into.  What the map costs: neighbouring lanes hold the same sample of consecutive points, so a wave's three
// `startsOut` stores land 48*S bytes apart, not coalesced at all -- accepted for a hook the tests and a firefly hunt use; a bake passes null,
// and the recorded measurement (profiles/r11_gather_query.md) is taken without it.
#pragma once

#include "tn_radiance.h"
#include "tn_query.h"

namespace tn {

enum GatherMode : uint32_t { kGatherCosine = 0, kGatherSphere = 1 };

struct GatherJob
{
    const void* points;     // tinsel_gather_point[first + count], 16-byte aligned
    void* startsOut;        // tinsel_path_start[(first + count)*samples], or null: the generated record of path (k, s) at k*samples + s
    void* out;              // float4[first + count]: k_gather_reduce's means
    uint32_t first;         // the point of the batch's point 0 (a query of more paths than a batch holds runs as several)
    uint32_t count;         // whole points of the batch: the batch's paths are slots [0, count*samples), slot = s*count + point
    uint32_t samples;
    uint32_t mode;          // GatherMode
};

// Sample s of a point: the generator Random(seed + s) after its two draws, and the direction they give (the point's second word: normal, seed).
// A pure function of the record and s: k_generate_gather starts the path with it, k_gather_sh_reduce derives it again for the basis.
TN_D V3 gather_direction(const WalkF4& pb, uint32_t s, uint32_t mode, Rng& rng)
{
    rng = Rng::seeded(__float_as_uint(pb.w) + s);
    const float u1 = rng.randf();
    const float u2 = rng.randf();
    if (mode == kGatherSphere)
        return uniform_sample_sphere(u1, u2);
    const V3 n(pb.x, pb.y, pb.z);
    V3 u, v;
    basis_from_vector(n, u, v);
    const V3 c = cosine_sample_hemisphere(u1, u2);
    return u*c.x + v*c.y + n*c.z;
}

__global__ __launch_bounds__(kBlock, 4) void k_generate_gather(SplitState ss, QueueCtl q, GatherJob job, const PrimBox* __restrict__ primBoxes, BinPrims bp)
{
    const GlobalF4 points = as_global(job.points) + (size_t)job.first*2u;
    const GlobalF4Out startsOut = (GlobalF4Out)(uintptr_t)job.startsOut + (size_t)job.first*job.samples*3u;
    generate_regions(ss, q, job.count*job.samples, primBoxes, bp, [&](uint32_t idx, PathRegs& p, uint32_t&) -> bool {
        const uint32_t s = idx/job.count, k = idx - s*job.count;
        const GlobalF4 rec = points + (size_t)k*2u;
        const WalkF4 pa = rec[0], pb = rec[1];
        Rng rng;
        const V3 d = gather_direction(pb, s, job.mode, rng);
        path_begin(p, V3(pa.x, pa.y, pa.z), d, pa.w, rng);
        if (job.startsOut)
        {
            const GlobalF4Out so = startsOut + ((size_t)k*job.samples + s)*3u;
            WalkF4 w0, w1, w2;
            w0.x = p.o.x; w0.y = p.o.y; w0.z = p.o.z; w0.w = p.time;
            w1.x = p.d.x; w1.y = p.d.y; w1.z = p.d.z; w1.w = 0.0f;
            w2.x = __uint_as_float(rng.s1); w2.y = __uint_as_float(rng.s2); w2.z = 0.0f; w2.w = 0.0f;
            so[0] = w0;
            so[1] = w1;
            so[2] = w2;
        }
        return true;
    });
}

// One lane per point of the batch: out[first + k] = (rad[k] + rad[count + k] + ... in ascending s, fp32) / (float)samples, word 3 zero.
// The additions stay in order; four loads are in flight ahead of them.
__global__ __launch_bounds__(kBlock) void k_gather_reduce(const float4* __restrict__ rad, GatherJob job)
{
    const uint32_t k = blockIdx.x*kBlock + threadIdx.x;
    if (k >= job.count)
        return;
    const GlobalF4 src = as_global(rad) + k;
    const size_t stride = job.count;
    float x = 0.0f, y = 0.0f, z = 0.0f;
    uint32_t s = 0;
    for (; s + 4 <= job.samples; s += 4)
    {
        const WalkF4 a = src[(size_t)s*stride], b = src[(size_t)(s + 1)*stride], c = src[(size_t)(s + 2)*stride], d = src[(size_t)(s + 3)*stride];
        x = x + a.x; y = y + a.y; z = z + a.z;
        x = x + b.x; y = y + b.y; z = z + b.z;
        x = x + c.x; y = y + c.y; z = z + c.z;
        x = x + d.x; y = y + d.y; z = z + d.z;
    }
    for (; s < job.samples; ++s)
    {
        const WalkF4 a = src[(size_t)s*stride];
        x = x + a.x; y = y + a.y; z = z + a.z;
    }
    const float count = (float)job.samples;
    WalkF4 mean;
    mean.x = x/count; mean.y = y/count; mean.z = z/count; mean.w = 0.0f;
    ((GlobalF4Out)(uintptr_t)job.out)[(size_t)job.first + k] = mean;
}

// The real orthonormal spherical harmonics of bands 0-2 on a unit direction, graphics convention, in the operation order include/tinsel_hip.h
// states (tinsel_amd.sh_basis mirrors it in float32): Y[0 .. (order+1)^2) are meant, all nine are computed.
constexpr int kShMaxCoeffs = 9;

TN_D void sh_basis(V3 d, float Y[kShMaxCoeffs])
{
    Y[0] = 0.28209479f;
    Y[1] = 0.48860251f*d.y;
    Y[2] = 0.48860251f*d.z;
    Y[3] = 0.48860251f*d.x;
    Y[4] = (1.0925484f*d.x)*d.y;
    Y[5] = (1.0925484f*d.y)*d.z;
    Y[6] = 0.31539157f*((3.0f*d.z)*d.z - 1.0f);
    Y[7] = (1.0925484f*d.x)*d.z;
    Y[8] = 0.54627422f*(d.x*d.x - d.y*d.y);
}

// One wave64 per point of the batch (the probe shape: few points, thousands of samples each -- one lane per point would leave the device
// idle, and the direction arithmetic belongs on every lane).  out[(first + k)*C + i] = (sum over s, ascending, fp32, of L_s * Y_i(d_s)) /
// (float)samples, word 3 zero, C = (order + 1)^2.  Per chunk of 64 samples: lane l takes sample 64*chunk + l, loads its radiance (the next
// chunk's load is in flight meanwhile), derives its direction again from the point record (gather_direction: nothing is stored per path)
// and the basis, and writes the 3C products to its row of `prod`; then lane j < 4C, which owns word j&3 of coefficient j>>2, adds its
// column down the rows -- strictly in s, into an accumulator that lives across the chunks.  Rows are 27 words whatever the order: an odd
// stride, so neither the row writes nor the column reads meet on a bank.  A group is one wave: the barriers are waits for LDS, no s_barrier.
constexpr int kShWave = 64;
constexpr int kShRow = 3*kShMaxCoeffs;

__global__ __launch_bounds__(kShWave) void k_gather_sh_reduce(const float4* __restrict__ rad, GatherJob job, int order)
{
    __shared__ float prod[kShWave*kShRow];
    const uint32_t k = blockIdx.x, lane = threadIdx.x;
    const GlobalF4 src = as_global(rad) + k;
    const size_t stride = job.count;
    const WalkF4 pb = (as_global(job.points) + ((size_t)job.first + k)*2u)[1];
    const uint32_t words = 4u*(uint32_t)((order + 1)*(order + 1));
    const bool sums = lane < words && (lane & 3u) != 3u;
    const float* const column = prod + (lane >> 2)*3u + (lane & 3u);
    float* const row = prod + lane*kShRow;
    float acc = 0.0f;
    WalkF4 next = 0.0f;
    if (lane < job.samples)
        next = src[(size_t)lane*stride];
    for (uint32_t base = 0; base < job.samples; base += kShWave)
    {
        const uint32_t s = base + lane, rows = min(job.samples - base, (uint32_t)kShWave);
        const WalkF4 L = next;
        if (s + kShWave < job.samples)
            next = src[(size_t)(s + kShWave)*stride];
        if (s < job.samples)
        {
            Rng rng;
            float Y[kShMaxCoeffs];
            sh_basis(gather_direction(pb, s, job.mode, rng), Y);
            const auto put = [&](int i) { row[3*i] = L.x*Y[i]; row[3*i + 1] = L.y*Y[i]; row[3*i + 2] = L.z*Y[i]; };
            put(0);
            if (order >= 1) { put(1); put(2); put(3); }
            if (order >= 2) { put(4); put(5); put(6); put(7); put(8); }
        }
        __syncthreads();
        if (sums)
        {
            if (rows == kShWave)
            {
#pragma unroll 16
                for (uint32_t i = 0; i < kShWave; ++i)
                    acc = acc + column[i*kShRow];
            }
            else
                for (uint32_t i = 0; i < rows; ++i)
                    acc = acc + column[i*kShRow];
        }
        __syncthreads();
    }
    if (lane < words)
        ((__attribute__((address_space(1))) float*)(uintptr_t)job.out)[((size_t)job.first + k)*words + lane] = sums ? acc/(float)job.samples : 0.0f;
}

} // namespace tn

// tn_denoise.h -- the feature-guided denoise stage (tinsel_hip_denoise*): a joint non-local-means filter on LINEAR radiance, guided by the
// planes tinsel_hip_render_features writes.  With the guide terms off it is NonLocalMeansFilter (nlm.cpp:35-77, k_nlm in tn_display.h) bit
// for bit; the albedo, normal and depth terms add to the exponent.  The statement is include/tinsel_hip.h's and tests/denoise_reference.py's.
//
//   k_denoise_prepare   per pixel: colour c = B.xyz/B.w, albedo a = A.xyz/A.w, mean normal n = N.xyz/N.w, depth z = D.x/D.z (0 where the
//                       divisor is 0 or the plane is absent), the demodulated colour u = c/max(a, floor) -- streaming, 64 B in, 48 B out
//   k_nlm_means         (tn_display.h) the patch means M = AverageFilter(U, patch_radius)
//   k_denoise           one workgroup per 32 x 8 pixel tile; the tile and its radius-wide halo of M, U and the guide values are staged into
//                       LDS once, every tap of the (2r+1)^2 window is then LDS reads
//
// LDS layout of k_denoise, per cell of the (32 + 2r) x (8 + 2r) region, 52 bytes in three float4 planes and one float plane:
//   sM = (M.xyz, z)   sU = (u.xyz, n.y)   sA = (a.xyz, n.x)   sNz = n.z         (sA only with ALBEDO or NORMAL, sNz only with NORMAL)
// 59,904 B at radius 8 with every plane (+ 256 B of expf's table): inside the 64 KB every kernel gets without asking, two workgroups per CU;
// 33 KB at radius 4 (four per CU).  A wave is 2 rows of 32 pixels and all its lanes read the same tap offset, so each ds_read_b128 lane
// group reads 16 consecutive 16-byte slots of one row and each ds_read_b32 half-wave 32 consecutive words: no bank conflict at any pitch
// (a 16 x 16 tile would have needed the pitch padded to a multiple of 16 cells for the same).  M.w is not staged: U.w is 0, so M.w is +0 and
// the dw*dw of LengthSq(Vec4) adds +0 to a sum of squares, which changes no bit.
// Cells outside the frame are neither written nor read: the window is clipped to the frame as in k_nlm.
//
// Exact arm only (tinsel_hip.hip): no FMA contraction, IEEE divide, expf as glibc evaluates it.
#pragma once

#include "tn_display.h"

#if TN_FAST
#error "tn_denoise.h is built under the parity contract only (tinsel_hip.hip)"
#endif

namespace tn {

constexpr int kDenoiseTileW = 32, kDenoiseTileH = 8;
constexpr int kDenoiseMaxRadius = 8, kDenoiseMaxPatch = 4;

struct DenoiseParams        // tinsel_hip_denoise_params, field for field
{
    int radius, patchRadius;
    float kColor, kAlbedo, kNormal, kDepth;
    int demodulate;
    float albedoFloor;
};

// dynamic LDS of k_denoise<MASK> at this radius
inline size_t denoise_lds_bytes(unsigned mask, int radius)
{
    const size_t cells = (size_t)(kDenoiseTileW + 2*radius)*(size_t)(kDenoiseTileH + 2*radius);
    return cells*(32u + ((mask & 3u) ? 16u : 0u) + ((mask & 2u) ? 4u : 0u));
}

TN_D float denoise_floor(float a, float floor) { return (a < floor) ? floor : a; }

// A, N, D: the planes that are there, else null.  ga = (a.xyz, z), gn = (n.xyz, 0), u = (u.xyz, 0)
__global__ __launch_bounds__(256) void k_denoise_prepare(const float4* __restrict__ beauty, const float4* __restrict__ A, const float4* __restrict__ N,
                                                         const float4* __restrict__ D, float4* __restrict__ u, float4* __restrict__ ga,
                                                         float4* __restrict__ gn, int n, int demodulate, float floor)
{
    const int i = blockIdx.x*256 + threadIdx.x;
    if (i >= n)
        return;
    const float4 b = beauty[i];
    float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), a = c, nn = c;
    if (b.w != 0.0f)
    {
        c.x = b.x/b.w; c.y = b.y/b.w; c.z = b.z/b.w;
    }
    if (A)
    {
        const float4 v = A[i];
        if (v.w != 0.0f)
        {
            a.x = v.x/v.w; a.y = v.y/v.w; a.z = v.z/v.w;
        }
    }
    if (N)
    {
        const float4 v = N[i];
        if (v.w != 0.0f)
        {
            nn.x = v.x/v.w; nn.y = v.y/v.w; nn.z = v.z/v.w;
        }
    }
    if (D)
    {
        const float4 v = D[i];
        if (v.z != 0.0f)
            a.w = v.x/v.z;
    }
    if (demodulate)
    {
        c.x = c.x/denoise_floor(a.x, floor);
        c.y = c.y/denoise_floor(a.y, floor);
        c.z = c.z/denoise_floor(a.z, floor);
    }
    u[i] = c;
    ga[i] = a;
    gn[i] = nn;
}

template <unsigned MASK>
__global__ __launch_bounds__(256) void k_denoise(const float4* __restrict__ means, const float4* __restrict__ u, const float4* __restrict__ ga,
                                                 const float4* __restrict__ gn, float4* __restrict__ out, int width, int height, DenoiseParams p)
{
    constexpr bool ALBEDO = (MASK & 1u) != 0, NORMAL = (MASK & 2u) != 0, DEPTH = (MASK & 4u) != 0;
    extern __shared__ float4 s_cells[];
    __shared__ unsigned long long s_exp[32];            // expf's table: (2r+1)^2 data-dependent reads per pixel
    if (threadIdx.x < 32)
        s_exp[threadIdx.x] = kExp2fTab[threadIdx.x];

    const int radius = p.radius;
    const int pitch = kDenoiseTileW + 2*radius, rows = kDenoiseTileH + 2*radius, cells = pitch*rows;
    float4* const sM = s_cells;
    float4* const sU = sM + cells;
    float4* const sA = sU + cells;
    float* const sNz = (float*)(sA + ((ALBEDO || NORMAL) ? cells : 0));
    const int x0 = (int)blockIdx.x*kDenoiseTileW - radius, y0 = (int)blockIdx.y*kDenoiseTileH - radius;

    for (int c = threadIdx.x; c < cells; c += 256)
    {
        const int ly = c/pitch, lx = c - ly*pitch;
        const int gx = x0 + lx, gy = y0 + ly;
        if (gx < 0 || gy < 0 || gx >= width || gy >= height)
            continue;
        const int g = gy*width + gx;
        float4 m = means[g], uu = u[g], a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (ALBEDO || DEPTH)
        {
            a = ga[g];
            m.w = a.w;
        }
        if (NORMAL)
        {
            const float4 nn = gn[g];
            a.w = nn.x;
            uu.w = nn.y;
            sNz[c] = nn.z;
        }
        sM[c] = m;
        sU[c] = uu;
        if (ALBEDO || NORMAL)
            sA[c] = a;
    }
    __syncthreads();

    const int x = (int)blockIdx.x*kDenoiseTileW + (threadIdx.x & 31);
    const int y = (int)blockIdx.y*kDenoiseTileH + (threadIdx.x >> 5);
    if (x >= width || y >= height)
        return;
    const int xlower = maxI(0, x - radius), xupper = minI(width - 1, x + radius);
    const int ylower = maxI(0, y - radius), yupper = minI(height - 1, y + radius);

    const int own = (y - y0)*pitch + (x - x0);
    const float4 mp = sM[own];
    float4 ap = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float npy = 0.0f, npz = 0.0f;
    if (ALBEDO || NORMAL)
        ap = sA[own];
    if (NORMAL)
    {
        npy = sU[own].w;
        npz = sNz[own];
    }

    float total = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (int fx = xlower; fx <= xupper; ++fx)
    {
        int q = (ylower - y0)*pitch + (fx - x0);
        for (int fy = ylower; fy <= yupper; ++fy, q += pitch)
        {
            const float4 m = sM[q], uu = sU[q];
            float dx = mp.x - m.x, dy = mp.y - m.y, dz = mp.z - m.z;
            float e = p.kColor*(dx*dx + dy*dy + dz*dz);
            if (ALBEDO || NORMAL)
            {
                const float4 a = sA[q];
                if (ALBEDO)
                {
                    dx = ap.x - a.x; dy = ap.y - a.y; dz = ap.z - a.z;
                    e = e + p.kAlbedo*(dx*dx + dy*dy + dz*dz);
                }
                if (NORMAL)
                {
                    dx = ap.w - a.w; dy = npy - uu.w; dz = npz - sNz[q];
                    e = e + p.kNormal*(dx*dx + dy*dy + dz*dz);
                }
            }
            if (DEPTH)
            {
                const float den = mp.w*mp.w + m.w*m.w;
                const float d = mp.w - m.w;
                e = e + p.kDepth*((den != 0.0f) ? d*d/den : 0.0f);
            }
            const float weight = m_expf_tab(-e, s_exp);
            sx += uu.x*weight; sy += uu.y*weight; sz += uu.z*weight;
            total += weight;
        }
    }
    const float rc = 1.0f/total;
    float4 o = make_float4(sx*rc, sy*rc, sz*rc, 1.0f);
    if (p.demodulate)           // (needs the albedo plane: judged by the host)
    {
        o.x = o.x*denoise_floor(ap.x, p.albedoFloor);
        o.y = o.y*denoise_floor(ap.y, p.albedoFloor);
        o.z = o.z*denoise_floor(ap.z, p.albedoFloor);
    }
    out[y*width + x] = o;
}

} // namespace tn

// tn_accumulate.h -- CpuRenderer::AddSample (render.cpp:401-445) as an order-preserving GATHER: k_accumulate (any filter), k_accumulate_tiled
// (16 x 16 pixel tiles, filter widths up to 2; its support form leaves out the adds of a weight that is +0 by construction), k_accumulate_piped
// (staging of the next pass overlapped with the gather).  Every kernel performs the same float operations in the same order, so what they
// share is stated once, ahead of them: a pass's candidate (raster position, clamped sample, footprint), its weights, the add, a tile's
// geometry, a shard's halo-tile setup and the radiance prefetch.  What is one kernel's own stays in it: which entries a thread stages and
// which window a pixel gathers, the support form's staging and its way back to the full window, the piped kernel's double buffer.
#pragma once

#include "tn_path_state.h"

namespace tn {

template <class Tab>
TN_D float filter_gauss_tab(float x, float falloff, float offset, const Tab& tab)     // same, expf table passed in
{
    return maxT(0.0f, float(m_expf_tab(-falloff*x*x, tab)) - offset);
}

TN_D float filter_gauss(float x, float falloff, float offset)      // Filter::Gaussian (render.h:29-32)
{
    return maxT(0.0f, float(m_expf(-falloff*x*x)) - offset);
}

// One candidate of a pass: the path generated at pixel (gx, gy), as AddSample sees it.

// camera_sample's raster position: the first two draws of the path's own stream (two LCG steps are cheaper than reading it back from the
// 16-B rngRaster record)
TN_D void raster_position(const FrameParams& fp, const uint32_t* __restrict__ passSeeds, int s, int gx, int gy, float& rx, float& ry)
{
    Rng rng = Rng::seeded((uint32_t)gx + (uint32_t)gy*(uint32_t)fp.width + passSeeds[fp.passBase + s]);
    const float x = rng.randf();
    const float y = rng.randf();
    rx = x + gx; ry = y + gy;
}

TN_D uint32_t pack_run(int start, int n) { return (uint32_t)start | (uint32_t)n << 16; }      // a run of columns / rows in one LDS word

// AddSample's splat footprint [int(x - fw), int(x + fw)] x [int(y - fw), int(y + fw)] cut to the frame (render.cpp:405-408): the columns
// [startX, startX + nX) and the rows [startY, startY + nY)
struct Footprint
{
    int startX, startY, nX, nY;
    TN_D bool covers(int px, int py) const { return (uint32_t)(px - startX) < (uint32_t)nX && (uint32_t)(py - startY) < (uint32_t)nY; }
};

TN_D Footprint splat_footprint(const FrameParams& fp, float rx, float ry)
{
    const float fw = fp.filterWidth;
    Footprint f;
    f.startX = maxI(0, int(rx - fw));
    f.startY = maxI(0, int(ry - fw));
    const int endX = minI(int(rx + fw), fp.width - 1);
    const int endY = minI(int(ry + fw), fp.height - 1);
    f.nX = maxI(0, endX - f.startX + 1);
    f.nY = maxI(0, endY - f.startY + 1);
    return f;
}

struct Candidate
{
    float rx, ry;       // raster position
    V3 c;               // the ALREADY CLAMPED sample (ClampLength is per path, render.cpp:412/431, not per covered pixel)
    Footprint f;
    // the LDS record of the tiled kernels: rgb, .w = bits(startX | nX << 16); beside it startY | nY << 16
    TN_D float4 record() const { return make_float4(c.x, c.y, c.z, __uint_as_float(pack_run(f.startX, f.nX))); }
    TN_D uint32_t rows() const { return pack_run(f.startY, f.nY); }
};

TN_D Candidate candidate_of_pass(const FrameParams& fp, const uint32_t* __restrict__ passSeeds, int s, int gx, int gy, const float4& ra)
{
    Candidate q;
    raster_position(fp, passSeeds, s, gx, gy, q.rx, q.ry);
    q.c = clamp_length(V3(ra.x, ra.y, ra.z), fp.clampLen);
    q.f = splat_footprint(fp, q.rx, q.ry);
    return q;
}

// The separable Gaussian weights of every footprint column and row of candidate q (each shared by the pixels of that column / row) into
// entry `le` of the two tables
template <int FOOT, int N, class Tab>
TN_D void stage_weights(const FrameParams& fp, const Candidate& q, float (&wx)[FOOT][N], float (&wy)[FOOT][N], int le, const Tab& tab)
{
    for (int kk = 0; kk < FOOT; ++kk)
    {
        if (kk < q.f.nX)
            wx[kk][le] = filter_gauss_tab((q.f.startX + kk) - q.rx, fp.filterFalloff, fp.filterOffset, tab);
        if (kk < q.f.nY)
            wy[kk][le] = filter_gauss_tab((q.f.startY + kk) - q.ry, fp.filterFalloff, fp.filterOffset, tab);
    }
}

// AddSample's add of staged candidate `le` to pixel (px, py), if its run of columns and its run of rows hold the pixel (render.cpp:414-443)
template <int FOOT, int N>
TN_D void add_candidate(float4& acc, int px, int py, bool gauss, const float4* s_c, const uint32_t* s_y, const float (&s_wx)[FOOT][N],
                        const float (&s_wy)[FOOT][N], int le)
{
    const float4 c = s_c[le];
    const uint32_t xm = __float_as_uint(c.w), ym = s_y[le];
    const uint32_t kx = (uint32_t)(px - (int)(xm & 0xffffu)), ky = (uint32_t)(py - (int)(ym & 0xffffu));
    if (kx >= (xm >> 16) || ky >= (ym >> 16))
        return;
    if (!gauss)
    {
        acc.x += c.x; acc.y += c.y; acc.z += c.z; acc.w += 1.0f;
    }
    else
    {
        const float w = s_wx[kx][le]*s_wy[ky][le];
        acc.x += c.x*w; acc.y += c.y*w; acc.z += c.z*w; acc.w += w;
    }
}

// k_accumulate: Pixel (px,py) visits the paths generated at pixels (i,j) in raster order, pass by pass, and
// adds the ones whose splat footprint [int(x-fw), int(x+fw)] x [int(y-fw), int(y+fw)] covers it --
// exactly the adds, in exactly the order, the serial oracle performs on that pixel.

__global__ __launch_bounds__(kBlock, 4) void k_accumulate(PathState ps, FrameParams fp, float4* __restrict__ accum, const uint32_t* __restrict__ passSeeds)
{
    const int npix = fp.width*fp.height;
    const int pix = blockIdx.x*kBlock + threadIdx.x;
    if (pix >= npix)
        return;
    const int py = pix/fp.width;
    const int px = pix - py*fp.width;

    const float fw = fp.filterWidth;
    // generating pixels (i,j) that can reach (px,py): i in [px-1-floor(fw), px+ceil(fw)]
    const int reachLo = 1 + (int)floorf(fw);
    const int reachHi = (int)ceilf(fw);
    const int i0 = maxI(0, px - reachLo), i1 = minI(fp.width - 1, px + reachHi);
    const int j0 = maxI(0, py - reachLo), j1 = minI(fp.height - 1, py + reachHi);

    float4 acc = accum[pix];

    for (int s = fp.accBegin; s < fp.accEnd; ++s)
    {
        for (int j = j0; j <= j1; ++j)
        {
            for (int i = i0; i <= i1; ++i)
            {
                if (!pixel_owned(fp, i, j))
                    continue;       // path not generated by this shard
                const size_t slot = slot_of(fp, s, i, j);
                float rx, ry;
                raster_position(fp, passSeeds, s, i, j, rx, ry);
                if (!splat_footprint(fp, rx, ry).covers(px, py))
                    continue;

                const float4 ra = ps.rad[slot];
                const V3 c = clamp_length(V3(ra.x, ra.y, ra.z), fp.clampLen);

                if (fp.filterType == 0)
                {
                    acc.x += c.x; acc.y += c.y; acc.z += c.z; acc.w += 1.0f;
                }
                else
                {
                    const float w = filter_gauss(px - rx, fp.filterFalloff, fp.filterOffset)*filter_gauss(py - ry, fp.filterFalloff, fp.filterOffset);
                    acc.x += c.x*w; acc.y += c.y*w; acc.z += c.z*w; acc.w += w;
                }
            }
        }
    }

    accum[pix] = acc;
}

// The tiled kernels: the same gather, one 16x16 pixel tile per block.  Per pass the block stages the (16 + halo)^2 candidate paths of its
// tile into LDS once instead of every pixel re-reading its 16 candidates from L2.  HBM traffic: one 16-B radiance record per path.  Same
// adds, same order; used when the footprint halo fits (filter width <= 2).

constexpr int kAccTile = 16;
constexpr int kAccMaxHalo = 5;      // reachLo + reachHi
constexpr int kAccSide = kAccTile + kAccMaxHalo;
constexpr int kAccEntries = kAccSide*kAccSide;
constexpr int kAccMaxFoot = 5;      // widest footprint (pixels per axis) for filter widths <= 2

// A block's tile and its candidates.  Sharded renders launch one block per tile that has candidate paths of THIS shard (tileList, built on
// the host: ownership depends on the pixel only); the other tiles have nothing to add in any pass, and with N shards they are most of the
// frame while the pass loop is N x longer.
struct AccTile
{
    int tx, ty;
    int reachLo, reachHi;   // generating pixels i that can reach pixel px: [px - reachLo, px + reachHi] = [px - 1 - floor(fw), px + ceil(fw)]
    int side;               // candidate entries per LDS row and column in use
    int ox, oy;             // frame coordinates of LDS entry (0,0)
    bool gauss;
};

TN_D AccTile tile_geometry(const FrameParams& fp, const int* __restrict__ tileList)
{
    const int tilesX = (fp.width + kAccTile - 1)/kAccTile;
    const int tile = tileList ? tileList[blockIdx.x] : (int)blockIdx.x;
    AccTile g;
    g.tx = tile % tilesX; g.ty = tile/tilesX;
    g.reachLo = 1 + (int)floorf(fp.filterWidth);
    g.reachHi = (int)ceilf(fp.filterWidth);
    g.side = kAccTile + g.reachLo + g.reachHi;
    g.ox = g.tx*kAccTile - g.reachLo; g.oy = g.ty*kAccTile - g.reachLo;
    g.gauss = fp.filterType != 0;
    return g;
}

// The K candidate entries a thread stages every pass: where in LDS, which path, whether the path is this shard's -- and their radiance, the
// NEXT pass's requested before the current pass is processed (nextRa: black until the first request, and for ever if the entry is not live).
template <int K>
struct AccEntries
{
    int le[K], gx[K], gy[K];
    bool live[K];
    float4 nextRa[K] = {};

    TN_D void request(const PathState& ps, const FrameParams& fp, int s)        // the radiance of batch pass s, if there is one
    {
        if (s < fp.accEnd)
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (live[k])
                    nextRa[k] = ps.rad[slot_of(fp, s, gx[k], gy[k])];
    }
    TN_D void rotate(const PathState& ps, const FrameParams& fp, int s, float4 (&curRa)[K])      // pass s's into curRa, pass s + 1's on its way
    {
#pragma unroll
        for (int k = 0; k < K; ++k)
            curRa[k] = nextRa[k];
        request(ps, fp, s + 1);
    }
};

// Is the path generated at (gx, gy) a candidate of this shard's at all?
TN_D bool candidate_live(const FrameParams& fp, int gx, int gy)
{
    return gx >= 0 && gy >= 0 && gx < fp.width && gy < fp.height && pixel_owned(fp, gx, gy);
}

// A shard's HALO tiles: the candidate window reaches an owned shard tile by a pixel or two, so only a strip of the tile's entries (or a
// corner) is this shard's and only a strip of its pixels has any candidate of this shard, in every pass (ownership is a function of the
// pixel).  Spread over the workgroup entry t, t + THREADS and pixel by pixel that is a lane or two of EVERY wave staging and gathering: a
// halo tile cost 0.7 of an inner one, and with 8 shards of 64-pixel tiles 20 of a shard tile's 36 accumulate tiles are halo while the pass
// loop is 8 x as long (profiles/r05_n_shard_tile.md).  So for a shard:
//   - the shard's own entries are handed out DENSELY (the t-th live entry to thread t): a strip is staged by one wave, and the entries
//     that are not the shard's are marked "covers nothing" once;
//   - pixels without a candidate of this shard are left alone altogether -- no gather, no load, no store -- and the tile's pixels are dealt
//     to the threads row by row or column by column, whichever leaves fewer waves with a pixel to do.
// A pixel's adds are its own thread's, in pass and raster order, whichever thread that is.

// The dense list: entry e, if live, behind the live entries of the lanes below and of the waves that came first (whole waves call this)
TN_D void list_live_entry(bool live, int e, int* list, int* count)
{
    const unsigned long long m = __ballot(live);
    int base = 0;
    if ((threadIdx.x & 63) == 0 && m != 0ull)
        base = atomicAdd(count, __popcll(m));
    base = __builtin_amdgcn_readfirstlane(base);
    if (live)
        list[base + (int)bits_below(m)] = e;
}

// Rows or columns: thread (lx, ly) takes pixel (lx, ly) of the tile or pixel (ly, lx); returns whether its pixel has a candidate of this
// shard.  flags[ey*stride + ex] != 0: entry (ex, ey) is live.  counts[0..1], zero on entry: waves with a pixel to do either way.  One
// barrier inside, which every thread of the block reaches; only the gatherers look at the flags.
TN_D bool deal_pixels(const FrameParams& fp, const AccTile& g, const uint32_t* flags, int stride, bool gatherer, int* counts, int& lx, int& ly)
{
    auto window_live = [&](int wx, int wy) {
        const int qx = g.tx*kAccTile + wx, qy = g.ty*kAccTile + wy;
        if (qx >= fp.width || qy >= fp.height)
            return false;
        const int a0 = maxI(0, qx - g.reachLo) - g.ox, a1 = minI(fp.width - 1, qx + g.reachHi) - g.ox;
        const int b0 = maxI(0, qy - g.reachLo) - g.oy, b1 = minI(fp.height - 1, qy + g.reachHi) - g.oy;
        uint32_t any = 0u;
        for (int j = b0; j <= b1; ++j)
            for (int i = a0; i <= a1; ++i)
                any |= flags[j*stride + i];
        return any != 0u;
    };
    const int cx = ly, cy = lx;                     // the same thread, column by column
    const bool byRow = gatherer && window_live(lx, ly);
    const bool byCol = gatherer && window_live(cx, cy);
    const bool waveRow = __ballot(byRow) != 0ull, waveCol = __ballot(byCol) != 0ull;
    if ((threadIdx.x & 63) == 0)
    {
        if (waveRow) atomicAdd(&counts[0], 1);
        if (waveCol) atomicAdd(&counts[1], 1);
    }
    __syncthreads();
    const bool columns = counts[1] < counts[0];
    if (columns) { lx = cx; ly = cy; }
    return columns ? byCol : byRow;
}

// k_accumulate_tiled
// SPAN = the candidate window's edge (reachLo + reachHi + 1: 3 for the default filter width 0.75, 4 for cornell's 1.0) as a compile-time
// constant: the gather loop is unrolled over the SPAN x SPAN window with no bounds -- candidates outside the frame are staged as
// "covers nothing", so clipping the window changes nothing -- in the same raster order; 0 = the window's bounds at run time.
// THREADS = kBlock, or 2*kBlock for frames of few tiles (one wave per SIMD or less: a pass is then as long as one thread's chain, and
// the second half of the workgroup -- no pixels of its own -- takes the second staging round off it).
//
// SUPPORT = the form for Gaussian filters whose weight is +0 by construction one pixel away from the sample (launch_accumulate decides: the
// filter's offset makes expf(a) - offset negative for every argument a <= argZero, and -falloff*1*1 <= argZero).  A path generated at pixel i
// then gives columns other than i and i + 1 the weight +0 whatever its footprint [int(r - fw), int(r + fw)] says, and x + (+0) is x: staging
// evaluates those two columns only (four expf instead of six, columns whose argument is <= argZero dropped from the run), and a pixel gathers the
// 2 x 2 candidates generated at {px - 1, px} x {py - 1, py} instead of its SPAN x SPAN window -- a subsequence of the same adds in the same
// order.  Two cases where adding +0 (or c*(+0)) is NOT a no-op send the block back to the full window, which stays here as it was:
//   - a sample with a non-finite component (0*inf is NaN in the reference) redoes that pass of the tile with the full window; every candidate
//     of the full window is loaded and looked at for this, also the ring no pixel of the tile gathers from in this form;
//   - an accumulator loaded with a -0 (-0 + +0 is +0) or a NaN component keeps the block on the full window for the whole launch.
template <int SPAN, int THREADS = kBlock, bool SUPPORT = false>
__global__ __launch_bounds__(THREADS, SUPPORT ? 6 : THREADS == kBlock ? 4 : 2) void k_accumulate_tiled(PathState ps, FrameParams fp, float4* __restrict__ accum,
                                                                const uint32_t* __restrict__ passSeeds, const int* __restrict__ tileList, float argZero)
{
    static_assert(!SUPPORT || SPAN == 3 || SPAN == 4, "the support form is for the compile-time windows");
    // LDS sized by what the window can hold: for the compile-time windows (filter widths up to 1) an edge of 16 + SPAN - 1 entries and at most
    // three footprint columns / rows per path (int(r + fw) - int(r - fw) + 1 <= 3) -- 14-16 KB a workgroup instead of 26.7, so the registers
    // (six waves per SIMD) and not the LDS (five workgroups per CU) set the occupancy of a kernel that waits half of its cycles
    constexpr int kSide = SPAN > 0 ? kAccTile + SPAN - 1 : kAccSide;
    constexpr int kEntries = kSide*kSide;
    // ... PLUS ONE: int(r + fw) - int(r - fw) + 1 is 2*fw + 1 in real arithmetic, but r + fw is a float sum -- where [r, r + fw] straddles a power of
    // two and r sits half an ulp below an integer, r + fw rounds UP to the next integer while r - fw does not (63.999996 + 2 -> 66.0, 63.999996 - 2 ->
    // 61.999996: six rows).  The reference then visits that extra row too (with a Gaussian weight of 0 when the filter's offset is the constructor's,
    // of whatever Filter::Gaussian says otherwise).  Until round 6 the tables had no entry for it and the gather read past them: one pixel in
    // 1e9 paths of the fuzz generator's scenes at 320 x 240 (scratch/fuzz_at_scale.py; tests/test_gpu_parity.py pins the case).
    constexpr int kFoot = (SPAN > 0 ? 3 : kAccMaxFoot) + 1;
    constexpr int kEnt = (kEntries + THREADS - 1)/THREADS;          // candidate entries a thread stages per pass
    // per candidate path of the tile: clamped sample, footprint [startX, startX+nX) x [startY, startY+nY)
    // and the separable Gaussian weights of its footprint columns / rows (each shared by up to 5 pixels)
    __shared__ float4 s_c[kEntries];                 // Candidate::record()
    __shared__ uint32_t s_y[kEntries];               // Candidate::rows()
    __shared__ float s_wx[kFoot][kEntries];
    __shared__ float s_wy[kFoot][kEntries];
    __shared__ unsigned long long s_exp[32];            // expf's table: six data-dependent reads per staged path
    __shared__ int s_redo;                              // SUPPORT: this pass of the tile has to be done with the full window
    if (threadIdx.x < 32)
        s_exp[threadIdx.x] = kExp2fTab[threadIdx.x];
    if (threadIdx.x == 0)
        s_redo = 0;
    __syncthreads();

    const AccTile g = tile_geometry(fp, tileList);
    const int side = g.side, reachLo = g.reachLo;

    // The (at most two) candidate entries this thread stages every pass
    AccEntries<kEnt> ent;
    bool entStage[kEnt];
    // SUPPORT: the 17 x 17 entries the pixels gather from -- generated at [tile - 1, tile + 15]^2 -- come first, the ring around them (looked at
    // for non-finite samples only) last, so that a wave stages one kind or the other
    constexpr int kCore = kAccTile + 1;
    bool entRing[kEnt];
    auto set_entry = [&](int k, int e) {
        int ex = e % side, ey = e/side;
        entRing[k] = false;
        if (SUPPORT)
        {
            const int a = reachLo - 1;                  // ring rows above (columns left of) the core; one below (right of) it: side == kCore + a + 1
            if (e < kCore*kCore)
            {
                ex = a + e % kCore; ey = a + e/kCore;
            }
            else
            {
                entRing[k] = true;
                int q = e - kCore*kCore;
                if (q < a*side) { ex = q % side; ey = q/side; }
                else if (q < (a + 1)*side) { ex = q - a*side; ey = side - 1; }
                else
                {
                    q -= (a + 1)*side;
                    const int c = q % (a + 1);
                    ex = c < a ? c : side - 1; ey = a + q/(a + 1);
                }
            }
        }
        ent.gx[k] = g.ox + ex; ent.gy[k] = g.oy + ey;
        ent.le[k] = ey*kSide + ex;
        ent.live[k] = e < side*side && candidate_live(fp, ent.gx[k], ent.gy[k]);
    };
#pragma unroll
    for (int k = 0; k < kEnt; ++k)
    {
        set_entry(k, threadIdx.x + k*THREADS);
        entStage[k] = threadIdx.x + k*THREADS < side*side;       // (entries outside the frame are staged as "covers nothing", every pass)
    }

    // Which pixel is this thread's, which entries does it stage?  Pixel by pixel, row by row (a wave = 4 rows of the tile) and entry
    // t, t + THREADS -- unless the tile is one of a shard's halo tiles (above)
    int lx = threadIdx.x % kAccTile, ly = (threadIdx.x/kAccTile) % kAccTile;
    bool mine = true;
    if (tileList)
    {
        __shared__ int s_count[3];                      // waves with a pixel to do (by rows, by columns); live entries
        int* s_list = reinterpret_cast<int*>(&s_wx[0][0]);      // (the weights are written by the passes: free until then)
        if (threadIdx.x < 3)
            s_count[threadIdx.x] = 0;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kEnt; ++k)
        {
            const int e = threadIdx.x + k*THREADS;
            if (e < side*side)
            {
                s_y[ent.le[k]] = ent.live[k] ? 1u : 0u;         // (the flags: free until the first pass is staged, like the list)
                s_c[ent.le[k]] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
            list_live_entry(ent.live[k], e, s_list, &s_count[2]);
        }
        __syncthreads();
        mine = deal_pixels(fp, g, s_y, kSide, threadIdx.x < kBlock, s_count, lx, ly);
        const int nLive = s_count[2];
#pragma unroll
        for (int k = 0; k < kEnt; ++k)
        {
            const int t = threadIdx.x + k*THREADS;
            entStage[k] = t < nLive;
            ent.live[k] = false;
            if (entStage[k])
                set_entry(k, s_list[t]);
        }
        __syncthreads();                                // (the flags and the list are staged over by the first pass)
    }
    ent.request(ps, fp, fp.accBegin);
    const int px = g.tx*kAccTile + lx, py = g.ty*kAccTile + ly;
    const bool inside = threadIdx.x < kBlock && px < fp.width && py < fp.height && mine;

    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (inside)
        acc = accum[py*fp.width + px];

    // this pixel's candidate window, in LDS coordinates (clipped to the frame like the reference's loops)
    const int i0 = maxI(0, px - reachLo) - g.ox, i1 = minI(fp.width - 1, px + g.reachHi) - g.ox;
    const int j0 = maxI(0, py - reachLo) - g.oy, j1 = minI(fp.height - 1, py + g.reachHi) - g.oy;

    // SUPPORT: an accumulator component that +0 changes (-0) or that is not a number: the whole launch of this block with the full window
    bool fullLaunch = false;
    if (SUPPORT)
    {
        auto fragile = [](float v) { const uint32_t b = __float_as_uint(v); return b == 0x80000000u || (b & 0x7fffffffu) > 0x7f800000u; };
        fullLaunch = __builtin_amdgcn_readfirstlane(__syncthreads_or(inside && (fragile(acc.x) || fragile(acc.y) || fragile(acc.z) || fragile(acc.w)))) != 0;
    }

    // one pass's candidates into LDS, every footprint column and row with its weight (the full window's staging)
    auto stage_full = [&](int s, const float4 (&curRa)[kEnt]) {
#pragma unroll
        for (int k = 0; k < kEnt; ++k)
        {
            if (!entStage[k])
                continue;
            const int le = ent.le[k];
            float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);     // nX == 0: covers nothing
            uint32_t ym = 0;
            if (ent.live[k])
            {
                const Candidate q = candidate_of_pass(fp, passSeeds, s, ent.gx[k], ent.gy[k], curRa[k]);
                c = q.record();
                ym = q.rows();
                if (g.gauss && !SUPPORT)
                    stage_weights(fp, q, s_wx, s_wy, le, s_exp);
                else if (g.gauss)
                {
                    // (the same weights one at a time: the support form comes here once in a blue moon and has no registers for more)
#pragma nounroll
                    for (int kk = 0; kk < 2*kFoot; ++kk)
                    {
                        const int col = kk >> 1;
                        if (col < ((kk & 1) ? q.f.nY : q.f.nX))
                        {
                            float* const w = (kk & 1) ? &s_wy[col][le] : &s_wx[col][le];
                            *w = filter_gauss_tab((((kk & 1) ? q.f.startY : q.f.startX) + col) - ((kk & 1) ? q.ry : q.rx), fp.filterFalloff, fp.filterOffset, s_exp);
                        }
                    }
                }
            }
            s_c[le] = c;
            s_y[le] = ym;
        }
    };

    // SUPPORT: the same candidates, of each one the columns gen and gen + 1 of its footprint (gen: the generating pixel's) whose expf argument
    // is above argZero (a run of 0, 1 or 2 columns: pack_run, its weights in s_wx[0..1]); the rows likewise
    auto stage_support = [&](int s, const float4 (&curRa)[kEnt]) {
        const float fw = fp.filterWidth;
        bool redo = false;
#pragma unroll
        for (int k = 0; k < kEnt; ++k)
        {
            if (!entStage[k])
                continue;
            const int gx = ent.gx[k], gy = ent.gy[k], le = ent.le[k];
            auto finite = [](float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; };
            if (entRing[k])
            {
                // no pixel gathers it in this form; in the full window it is a candidate, and 0*inf is not 0
                if (ent.live[k])
                {
                    const V3 cl = clamp_length(V3(curRa[k].x, curRa[k].y, curRa[k].z), fp.clampLen);
                    redo = redo || !(finite(cl.x) && finite(cl.y) && finite(cl.z));
                }
                continue;
            }
            float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            uint32_t ym = 0;
            if (ent.live[k])
            {
                const Candidate q = candidate_of_pass(fp, passSeeds, s, gx, gy, curRa[k]);        // (its footprint: the axis loop's own start and end)
                redo = redo || !(finite(q.c.x) && finite(q.c.y) && finite(q.c.z));

                // x, then y -- one after the other (a loop the compiler is told to leave alone: four expf in flight at once cost the sixth wave)
                uint32_t run[2];
#pragma nounroll
                for (int ax = 0; ax < 2; ++ax)
                {
                    const int gen = ax ? gy : gx, limit = (ax ? fp.height : fp.width) - 1;
                    const float r = ax ? q.ry : q.rx;
                    float* const w = ax ? &s_wy[0][le] : &s_wx[0][le];
                    const int start = maxI(0, int(r - fw)), end = minI(int(r + fw), limit);
                    // (the arguments as Filter::Gaussian forms them: -falloff*x*x with x = column - r)
                    const float d0 = gen - r, d1 = (gen + 1) - r, dLo = (gen - 1) - r, dHi = (gen + 2) - r;
                    const float a0 = -fp.filterFalloff*d0*d0, a1 = -fp.filterFalloff*d1*d1;
                    const bool in0 = gen >= start && gen <= end && a0 > argZero;
                    const bool in1 = gen + 1 >= start && gen + 1 <= end && a1 > argZero;
                    const float e1 = maxT(0.0f, float(m_expf_tab(a1, s_exp)) - fp.filterOffset);
                    w[kEntries] = e1;
                    const float e0 = maxT(0.0f, float(m_expf_tab(a0, s_exp)) - fp.filterOffset);
                    w[0] = in0 ? e0 : e1;
                    // the columns next to the pair are |x| >= 1 away, so the host's rule puts their arguments at or below argZero: checked all the same
                    redo = redo || -fp.filterFalloff*dLo*dLo > argZero || -fp.filterFalloff*dHi*dHi > argZero;
                    run[ax] = pack_run(in0 ? gen : gen + 1, (in0 ? 1 : 0) + (in1 ? 1 : 0));
                }
                ym = run[1];
                c = make_float4(q.c.x, q.c.y, q.c.z, __uint_as_float(run[0]));
            }
            s_c[le] = c;
            s_y[le] = ym;
        }
        if (redo)
            s_redo = 1;
    };

    for (int s = fp.accBegin; s < fp.accEnd; ++s)
    {
        float4 curRa[kEnt];
        ent.rotate(ps, fp, s, curRa);

        bool full = !SUPPORT || fullLaunch;
        if (SUPPORT && !full)
        {
            stage_support(s, curRa);
            __syncthreads();
            full = __builtin_amdgcn_readfirstlane(s_redo) != 0;
            if (full)
                __syncthreads();                        // (everyone has read the flag and is done with this staging)
        }
        if (full)
        {
            stage_full(s, curRa);
            if (SUPPORT && threadIdx.x == 0)
                s_redo = 0;
            __syncthreads();
        }

        auto add = [&](int le) { add_candidate(acc, px, py, g.gauss, s_c, s_y, s_wx, s_wy, le); };
        if (inside)
        {
            if (SUPPORT && !full)
            {
                // the candidates generated at {px - 1, px} x {py - 1, py}: LDS entry (lx + reachLo - 1, ly + reachLo - 1) onwards
#pragma unroll
                for (int dj = 0; dj < 2; ++dj)
#pragma unroll
                    for (int di = 0; di < 2; ++di)
                        add((ly + reachLo - 1 + dj)*kSide + lx + reachLo - 1 + di);
            }
            else if (SUPPORT)
            {
                // (the full window in the support form's kernel: rare, so a plain loop)
#pragma nounroll
                for (int dj = 0; dj < SPAN; ++dj)
#pragma nounroll
                    for (int di = 0; di < SPAN; ++di)
                        add((ly + dj)*kSide + lx + di);
            }
            else if (SPAN > 0)
            {
                // the window of pixel (lx, ly) starts at LDS entry (lx, ly): px - reachLo - ox == lx
#pragma unroll
                for (int dj = 0; dj < SPAN; ++dj)
#pragma unroll
                    for (int di = 0; di < SPAN; ++di)
                        add((ly + dj)*kSide + lx + di);
            }
            else
            {
                for (int j = j0; j <= j1; ++j)
                    for (int i = i0; i <= i1; ++i)
                        add(j*kSide + i);
            }
        }
        __syncthreads();
    }

    if (inside)
        accum[py*fp.width + px] = acc;
}

// k_accumulate_piped: the same adds for launches of FEW tiles, where a tile's pass loop -- stage the pass's candidates, barrier, gather,
// barrier, one pass after the other -- is what the launch lasts: a small frame (a wave per SIMD or less), or a shard of N, whose pass
// loop is N x as long over 1/N of the tiles (8 shards of cornell 1024^2: 160 passes x 3.5 us whatever else was changed; calls o-p).
// Ten waves per tile: waves 4-9 stage pass s + 1 into one half of a double buffer while waves 0-3 gather pass s from the other; one
// barrier per pass, and a pass lasts as long as the longer of the two instead of their sum.  A pixel's adds are still one thread's, in
// pass and raster order.  Entries that cover nothing in any pass (outside the frame, another shard's) are marked so once, in both
// halves; every tile goes through the halo-tile setup (own entries dense, pixels without a candidate left alone, rows or columns).
constexpr int kAccPipeStagers = 384;        // >= 19 x 19 entries (filter widths up to 1): one entry per staging thread
constexpr int kAccPipeThreads = kBlock + kAccPipeStagers;

template <int SPAN>
__global__ __launch_bounds__(kAccPipeThreads, 2) void k_accumulate_piped(PathState ps, FrameParams fp, float4* __restrict__ accum,
                                                                     const uint32_t* __restrict__ passSeeds, const int* __restrict__ tileList)
{
    static_assert(SPAN == 3 || SPAN == 4, "the compile-time windows only (filter widths up to 1)");
    constexpr int kEnt = (kAccEntries + kAccPipeStagers - 1)/kAccPipeStagers;
    // footprint columns / rows a path can have: int(r + fw) - int(r - fw) + 1 <= 3 for the filter widths of SPAN 3 and 4 (fw <= 1)
    constexpr int kFoot = 3 + 1;                        // (+ 1: the row / column a rounded-up r + fw adds, k_accumulate_tiled above)
    __shared__ float4 s_c[2][kAccEntries];              // Candidate::record()
    __shared__ uint32_t s_y[2][kAccEntries];            // Candidate::rows()
    __shared__ float s_wx[2][kFoot][kAccEntries];
    __shared__ float s_wy[2][kFoot][kAccEntries];
    __shared__ unsigned long long s_exp[32];
    __shared__ int s_count[3];                          // waves with a pixel to do (by rows, by columns); live entries
    if (threadIdx.x < 32)
        s_exp[threadIdx.x] = kExp2fTab[threadIdx.x];
    if (threadIdx.x < 3)
        s_count[threadIdx.x] = 0;

    const AccTile g = tile_geometry(fp, tileList);
    const int side = g.side;
    const bool stager = threadIdx.x >= kBlock;
    const int sid = (int)threadIdx.x - kBlock;          // stagers: 0 .. kAccPipeStagers - 1

    // every thread marks entries "cover nothing" in both halves and flags the live ones; the live entries are listed densely
    int* s_list = reinterpret_cast<int*>(&s_wx[1][0][0]);      // (free until the second pass is staged)
    for (int e = threadIdx.x; e < kAccEntries; e += kAccPipeThreads)
    {
        s_c[0][e] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        s_c[1][e] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        s_y[0][e] = 0u;
        s_y[1][e] = 0u;
    }
    __syncthreads();
    for (int e0 = 0; e0 < side*side; e0 += kAccPipeThreads)
    {
        const int e = e0 + (int)threadIdx.x;
        const int ex = e % side, ey = e/side;
        const bool live = e < side*side && candidate_live(fp, g.ox + ex, g.oy + ey);
        list_live_entry(live, e, s_list, &s_count[2]);
        if (live)
            s_y[1][ey*kAccSide + ex] = 1u;              // (the flag: read below, staged over by the second pass)
    }
    __syncthreads();
    const int nLive = s_count[2];

    // gatherers: which pixel
    int lx = threadIdx.x % kAccTile, ly = (threadIdx.x/kAccTile) % kAccTile;
    const bool mine = deal_pixels(fp, g, s_y[1], kAccSide, !stager, s_count, lx, ly);
    // stagers: which entries
    AccEntries<kEnt> ent;
#pragma unroll
    for (int k = 0; k < kEnt; ++k)
    {
        const int t = sid + k*kAccPipeStagers;
        ent.live[k] = stager && t < nLive;
        ent.le[k] = 0; ent.gx[k] = 0; ent.gy[k] = 0;
        if (ent.live[k])
        {
            const int e = s_list[t];
            const int ex = e % side, ey = e/side;
            ent.gx[k] = g.ox + ex; ent.gy[k] = g.oy + ey;
            ent.le[k] = ey*kAccSide + ex;
        }
    }
    ent.request(ps, fp, fp.accBegin);
    __syncthreads();                                    // (flags and list read by everyone)
    for (int e = threadIdx.x; e < kAccEntries; e += kAccPipeThreads)
        s_y[1][e] = 0u;                                 // the flags go; the barrier of the first staging orders this before any write of half 1

    const int px = g.tx*kAccTile + lx, py = g.ty*kAccTile + ly;
    const bool inside = !stager && mine;                // (deal_pixels: inside the frame)
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (inside)
        acc = accum[py*fp.width + px];

    // stage pass s into half h (stagers)
    auto stage = [&](int s, int h) {
        float4 curRa[kEnt];
        ent.rotate(ps, fp, s, curRa);
#pragma unroll
        for (int k = 0; k < kEnt; ++k)
        {
            if (!ent.live[k])
                continue;
            const int le = ent.le[k];
            const Candidate q = candidate_of_pass(fp, passSeeds, s, ent.gx[k], ent.gy[k], curRa[k]);
            if (g.gauss)
                stage_weights(fp, q, s_wx[h], s_wy[h], le, s_exp);
            s_c[h][le] = q.record();
            s_y[h][le] = q.rows();
        }
    };

    __syncthreads();
    if (stager && fp.accBegin < fp.accEnd)
        stage(fp.accBegin, 0);
    __syncthreads();

    for (int s = fp.accBegin; s < fp.accEnd; ++s)
    {
        const int h = (s - fp.accBegin) & 1;
        if (stager)
        {
            if (s + 1 < fp.accEnd)
                stage(s + 1, h ^ 1);
        }
        else if (inside)
        {
            // the window of pixel (lx, ly) starts at LDS entry (lx, ly), as in k_accumulate_tiled
#pragma unroll
            for (int dj = 0; dj < SPAN; ++dj)
#pragma unroll
                for (int di = 0; di < SPAN; ++di)
                    add_candidate(acc, px, py, g.gauss, s_c[h], s_y[h], s_wx[h], s_wy[h], (ly + dj)*kAccSide + lx + di);
        }
        __syncthreads();
    }

    if (inside)
        accum[py*fp.width + px] = acc;
}

} // namespace tn

// plane_pairs_host.cpp -- tn_plane.h (the text the kernels compile) built for the host, on its own: the paired plane test against two
// IntersectRayPlane calls, bit for bit.  tests/test_plane_pairs.py builds it with -ffp-contract=off and runs it as a child process.
//
//   plane_pairs_host [log2 of the number of random triples, default 28] [threads, default 8]
//
// For every (origin, direction, pair) it compares, by their bits: the hit flags, t, the chosen plane and its normal.  A triple whose
// paired form says `both` takes the two calls in the kernel too (trace_flat's wave-uniform fallback); it is counted, and checked to be
// the only place where both planes of a pair are hit.  Prints one summary line; exit status 1 on the first mismatch (printed).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <thread>
#include <vector>

#include "tn_plane.h"

namespace {

uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

struct Rng
{
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed*0x9E3779B97F4A7C15ull + 0xD1B54A32D192ED03ull) {}
    uint64_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s*0x2545F4914F6CDD1Dull; }
    uint32_t u32() { return (uint32_t)(next() >> 32); }
    float unit() { return (float)(u32() >> 8)*(1.0f/16777216.0f); }          // [0, 1)
    float sym(float r) { return (unit()*2.0f - 1.0f)*r; }
};

struct Counts { unsigned long long n = 0, both = 0, hitA = 0, hitB = 0, none = 0; };

std::atomic<int> g_failed(0);

// one triple; false (and a printed line) on a mismatch
bool check(const float o[3], const float d[3], const float A[4], const float B[4], Counts& c)
{
    float tA = 0.0f, tB = 0.0f;
    const bool hA = tn::ray_plane_eq(o[0], o[1], o[2], d[0], d[1], d[2], A[0], A[1], A[2], A[3], tA);
    const bool hB = tn::ray_plane_eq(o[0], o[1], o[2], d[0], d[1], d[2], B[0], B[1], B[2], B[3], tB);
    const tn::PlanePair pp = tn::plane_pair_pick(o[0], o[1], o[2], d[0], d[1], d[2], A[0], A[1], A[2], A[3], B[3]);
    ++c.n;
    bool ok = true;
    if (pp.both)
        ++c.both;           // (the kernel runs the two calls above for this wave)
    else
    {
        float t = 0.0f;
        const bool h = tn::plane_pair_hit(pp, t);
        const float* chosen = pp.b ? B : A;
        if (hA && hB) ok = false;                                   // two hits are the fallback's
        else if (h != (hA || hB)) ok = false;
        else if (h && (pp.b != hB || bits(t) != bits(hB ? tB : tA))) ok = false;
        else if (h && (bits(chosen[0]) != bits(hB ? B[0] : A[0]) || bits(chosen[1]) != bits(hB ? B[1] : A[1]) || bits(chosen[2]) != bits(hB ? B[2] : A[2]))) ok = false;
        c.hitA += h && !pp.b; c.hitB += h && pp.b; c.none += !h;
    }
    if (!ok && g_failed.fetch_add(1) == 0)
        printf("MISMATCH o=%08x %08x %08x d=%08x %08x %08x A=%08x %08x %08x %08x B=%08x %08x %08x %08x: two calls %d %08x / %d %08x, pair b=%d q=%08x den=%08x\n",
               bits(o[0]), bits(o[1]), bits(o[2]), bits(d[0]), bits(d[1]), bits(d[2]), bits(A[0]), bits(A[1]), bits(A[2]), bits(A[3]),
               bits(B[0]), bits(B[1]), bits(B[2]), bits(B[3]), (int)hA, bits(tA), (int)hB, bits(tB), (int)pp.b, bits(pp.q), bits(pp.den));
    return ok;
}

// B from A by the host's pairing rule: every normal component negated bitwise, a zero with either sign
void opposite(const float A[4], float B[4], Rng& r)
{
    for (int k = 0; k < 3; ++k)
        B[k] = (A[k] == 0.0f && (r.u32() & 1u)) ? from_bits(r.u32() & 0x80000000u) : from_bits(bits(A[k]) ^ 0x80000000u);
}

float finite_bits(Rng& r)
{
    for (;;)
    {
        const uint32_t u = r.u32();
        if ((u & 0x7f800000u) != 0x7f800000u)
            return from_bits(u);
    }
}

void random_triples(uint64_t seed, unsigned long long count, Counts& c)
{
    Rng r(seed);
    float o[3], d[3], A[4], B[4];
    for (unsigned long long i = 0; i < count && !g_failed.load(std::memory_order_relaxed); ++i)
    {
        const uint32_t kind = r.u32();
        // the pair: axis-aligned (cornell's, glass's), scaled, oblique, or any finite bits
        switch (kind & 3u)
        {
        case 0: { const int ax = (int)(r.u32()%3u); const float s = (r.u32() & 1u) ? 1.0f : -1.0f;
                  for (int k = 0; k < 3; ++k) A[k] = k == ax ? s : ((r.u32() & 1u) ? 0.0f : -0.0f); break; }
        case 1: { const int ax = (int)(r.u32()%3u); const float s = r.sym(4.0f);
                  for (int k = 0; k < 3; ++k) A[k] = k == ax ? s : 0.0f; break; }
        case 2: for (int k = 0; k < 3; ++k) A[k] = r.sym(1.0f); break;
        default: for (int k = 0; k < 3; ++k) A[k] = finite_bits(r); break;
        }
        opposite(A, B, r);
        switch ((kind >> 2) & 3u)
        {
        case 0: A[3] = r.sym(2.0f); B[3] = r.sym(2.0f); break;
        case 1: A[3] = r.unit()*2.0f; B[3] = r.unit()*2.0f; break;             // a slab around the origin
        case 2: A[3] = r.sym(2.0f); B[3] = -A[3]; break;                       // w_A = -w_B: the same plane from both sides
        default: A[3] = finite_bits(r); B[3] = finite_bits(r); break;
        }
        // the origin: anywhere near, on plane A, or any bits (NaN and infinity too)
        switch ((kind >> 4) & 3u)
        {
        case 0: case 1: for (int k = 0; k < 3; ++k) o[k] = r.sym(3.0f); break;
        case 2: {
            for (int k = 0; k < 3; ++k) o[k] = r.sym(3.0f);
            const float nn = A[0]*A[0] + A[1]*A[1] + A[2]*A[2];
            const float s = (A[0]*o[0] + A[1]*o[1] + A[2]*o[2] + A[3])/nn;
            for (int k = 0; k < 3; ++k) o[k] -= s*A[k];                        // (on the plane up to rounding: numerators around zero)
            break; }
        default: for (int k = 0; k < 3; ++k) o[k] = from_bits(r.u32()); break;
        }
        // the direction: unit-ish, with exact and signed zeros, or any bits
        switch ((kind >> 6) & 3u)
        {
        case 0: case 1: for (int k = 0; k < 3; ++k) d[k] = r.sym(1.0f); break;
        case 2: for (int k = 0; k < 3; ++k) { const uint32_t z = r.u32()%3u; d[k] = z == 0 ? 0.0f : z == 1 ? -0.0f : r.sym(1.0f); } break;
        default: for (int k = 0; k < 3; ++k) d[k] = from_bits(r.u32()); break;
        }
        check(o, d, A, B, c);
    }
}

// every combination of a few special values: zero and signed-zero direction components, origins on a plane and outside the slab,
// denormal numerators, w_A = -w_B, normals scaled by 2 and down into the denormals
void directed(Counts& c)
{
    const float normals[][3] = { { 0.0f, 1.0f, 0.0f }, { -0.0f, -1.0f, 0.0f }, { 1.0f, 0.0f, -0.0f }, { 0.0f, 2.0f, 0.0f }, { 0.0f, 0.0f, -0.5f },
                                 { 0.6f, 0.8f, 0.0f }, { 1e-20f, 0.0f, 0.0f }, { 0.0f, 1e-39f, 0.0f }, { 0.0f, 0.0f, 0.0f }, { 3e38f, 3e38f, 0.0f } };
    const float ws[] = { 0.0f, -0.0f, 1.0f, -1.0f, 2.0f, 1e-40f, -1e-40f, 1e-4f, 3e38f };
    const float os[] = { 0.0f, -0.0f, 1.0f, -1.0f, 0.5f, 2.0f, -3.0f, 1e-40f, -1e-45f, 1e-20f, 1e6f };
    const float ds[] = { 0.0f, -0.0f, 1.0f, -1.0f, 1e-40f, -1e-45f, 0.70710678f, 3e38f };
    Rng r(7);
    float o[3], d[3], A[4], B[4];
    for (const auto& n : normals)
        for (const float wa : ws)
            for (const float wb : ws)
                for (const float oa : os)
                    for (const float ob : os)
                        for (const float da : ds)
                            for (const float db : ds)
                                for (int perm = 0; perm < 3; ++perm)
                                {
                                    A[0] = n[0]; A[1] = n[1]; A[2] = n[2]; A[3] = wa; B[3] = wb;
                                    opposite(A, B, r);
                                    o[perm] = oa; o[(perm + 1)%3] = ob; o[(perm + 2)%3] = 0.25f;
                                    d[perm] = da; d[(perm + 1)%3] = db; d[(perm + 2)%3] = -0.0f;
                                    check(o, d, A, B, c);
                                    d[(perm + 2)%3] = 0.5f;
                                    check(o, d, A, B, c);
                                }
}

} // namespace

int main(int argc, char** argv)
{
    const int log2n = argc > 1 ? atoi(argv[1]) : 28;
    const int threads = argc > 2 ? atoi(argv[2]) : 8;
    if (log2n < 0 || log2n > 40 || threads < 1 || threads > 256)
        return 2;
    Counts dc;
    directed(dc);
    const unsigned long long total = 1ull << log2n, each = (total + (unsigned long long)threads - 1)/(unsigned long long)threads;
    std::vector<Counts> cs((size_t)threads);
    std::vector<std::thread> pool;
    for (int k = 0; k < threads; ++k)
        pool.emplace_back(random_triples, (uint64_t)(k + 1), each, std::ref(cs[(size_t)k]));
    for (std::thread& t : pool)
        t.join();
    Counts c;
    for (const Counts& k : cs) { c.n += k.n; c.both += k.both; c.hitA += k.hitA; c.hitB += k.hitB; c.none += k.none; }
    printf("directed %llu (both ahead %llu, A %llu, B %llu, no hit %llu) random %llu (both ahead %llu, A %llu, B %llu, no hit %llu) mismatches %d\n",
           dc.n, dc.both, dc.hitA, dc.hitB, dc.none, c.n, c.both, c.hitA, c.hitB, c.none, g_failed.load());
    return g_failed.load() ? 1 : 0;
}

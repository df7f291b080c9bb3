// tn_plane.h -- IntersectRayPlane, and the same test for two OPPOSING planes with one division.
//
// Plain scalar fp32, no vector types: the device compiles this text inside tn_isect.h, and a host compiler builds it on its own
// (tests/plane_pairs_host.cpp compares the paired form with two IntersectRayPlane calls bit for bit).  Like everything in tn_isect.h
// it must be compiled with -ffp-contract=off: the operation order is the reference's.
#pragma once

#include <stdint.h>
#include <string.h>

#ifndef TN_HD
#define TN_HD inline
#endif

namespace tn {

TN_HD uint32_t plane_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// IntersectRayPlane (intersection.h:85-99); Dot(Vec4,Vec4) keeps the w term (maths.h:331)
TN_HD bool ray_plane_eq(float ox, float oy, float oz, float dx, float dy, float dz, float px, float py, float pz, float pw, float& t)
{
    float d = px*dx + py*dy + pz*dz + pw*0.0f;
    if (d == 0.0f)
        return false;
    t = -(px*ox + py*oy + pz*oz + pw*1.0f)/d;
    return t > 0.0f;
}

// Two planes A and B of the plane table whose normals are each other's negation component by component (bitwise, or both components
// are zeros of any sign) and whose eight coefficients are finite: the host's pairing rule (plane_pair_ok, tn_host_scene.h).  For such a
// pair IntersectRayPlane(B) is determined by A's two dot products (DESIGN.md section 5 has the argument in full):
//   denominator  den_B is the term-by-term negation of den_A -- a negated product is exact and round-to-nearest is symmetric under
//                negation, so den_B == -den_A; the signed zeros pw*0.0f adds only matter where the sum is a zero, and then both planes
//                miss by `d == 0.0f`
//   numerator    by the same argument n_B.o == -(n_A.o), so num_B = -S + w_B*1.0f with S = n_A.o
//   quotient     t_B = -num_B/den_B = (-num_B)/(-den_A), which is the quotient num_B/den_A
//   skipped      a quotient whose operands differ in sign, or whose numerator is a zero, is negative or a zero: never `> 0`
// So only a plane whose numerator and den_A are non-zero and of equal sign can be hit ("ahead"), and a ray that starts between
// the two has at most one of them ahead.  PlanePair holds what ONE division then needs; `both` says that this ray has both ahead (its
// origin lies outside the slab, or the planes face away from each other) and must take the two IntersectRayPlane calls instead.
struct PlanePair
{
    float den;      // den_A
    float q;        // the chosen plane's numerator over den_A: -num_A, or num_B
    bool b;         // B is the chosen plane
    bool both;
};

TN_HD PlanePair plane_pair_pick(float ox, float oy, float oz, float dx, float dy, float dz, float ax, float ay, float az, float aw, float bw)
{
    PlanePair r;
    r.den = ax*dx + ay*dy + az*dz + aw*0.0f;
    const float S = ax*ox + ay*oy + az*oz;
    const float qa = -(S + aw*1.0f);
    const float qb = -S + bw*1.0f;
    // "Ahead" by the sign bits alone: equal sign bits is all a plane needs to be a candidate.  That flags a few planes that cannot be hit
    // either (a zero numerator, a NaN) -- harmless: flagged alone, such a plane's own quotient is computed and is not > 0 while the other
    // plane, not flagged, cannot be hit; flagged beside the other plane, the ray takes the two calls.
    const uint32_t sd = plane_bits(r.den), xa = plane_bits(qa) ^ sd, xb = plane_bits(qb) ^ sd;
    r.both = (int32_t)(xa | xb) >= 0;
    r.b = (int32_t)xb >= 0;
    r.q = r.b ? qb : qa;            // neither ahead: A's own quotient, which is not > 0
    return r;
}

// the chosen plane's IntersectRayPlane: its `d == 0.0f` (den_B is a zero exactly where den_A is) and its `t > 0.0f`
TN_HD bool plane_pair_hit(const PlanePair& r, float& t)
{
    if (r.den == 0.0f)
        return false;
    t = r.q/r.den;
    return t > 0.0f;
}

} // namespace tn

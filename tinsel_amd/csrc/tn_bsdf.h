// tn_bsdf.h -- the Disney uber-BSDF of the reference (src/disney.h), evaluated from the
// pre-digested Mat128 record.  Material-only sub-expressions that the reference evaluates
// in double on the host (Cdlum/Ctint/Cspec0 disney.h:306-310, the clearcoat alpha :387,
// the IOR scene.h:72-78) are computed once in host_scene.cpp with the same expressions.
#pragma once

#include "tn_scene.h"

namespace tn {

enum BsdfType : int { kReflected = 0, kTransmitted = 1, kSpecular = 2 };   // disney.h:27-32

struct Mat
{
    V3 emission, color, absorption, cspec0, sqrtColor;
    float ior, metallic, subsurface, roughness, transmission, clearcoat, clearcoatAlpha, clearcoatA2, clearcoatLogA2, area;
    int lightSamples;
    float rcpArea, rcpLightSamples, cbsdf, clight;      // Mat128: the MIS constants divided on the host
};

TN_D Mat load_mat(const Mat128* mats, int idx)
{
    const float4* p = reinterpret_cast<const float4*>(mats + idx);
    float4 a = p[0], b = p[1], c = p[2], d = p[3], e = p[4], f = p[5], g = p[6], h = p[7];
    Mat m;
    m.emission = V3(a.x, a.y, a.z); m.ior = a.w;
    m.color = V3(b.x, b.y, b.z); m.metallic = b.w;
    m.absorption = V3(c.x, c.y, c.z); m.subsurface = c.w;
    m.cspec0 = V3(d.x, d.y, d.z); m.roughness = d.w;
    m.sqrtColor = V3(e.x, e.y, e.z); m.transmission = e.w;
    m.clearcoat = f.x; m.clearcoatAlpha = f.y; m.area = f.z; m.lightSamples = __float_as_int(f.w);
    m.clearcoatA2 = g.x; m.clearcoatLogA2 = g.y;
    m.rcpArea = g.z; m.rcpLightSamples = g.w; m.cbsdf = h.x; m.clight = h.y;
    return m;
}

// Refract (disney.h:34-47)
TN_D bool refract(V3 wi, V3 n, float eta, V3& wt)
{
    float cosThetaI = dot(n, wi);
    float sin2ThetaI = maxT(0.0f, 1.0f - cosThetaI*cosThetaI);
    float sin2ThetaT = eta*eta*sin2ThetaI;
    if (sin2ThetaT >= 1)
        return false;
    float cosThetaT = sqrtf_cr(1.0f - sin2ThetaT);
    wt = eta*(-wi) + (eta*cosThetaI - cosThetaT)*n;
    return true;
}

TN_D float schlick_fresnel(float u)        // disney.h:49-54
{
    float m = clampT(1 - u, 0.0f, 1.0f);
    float m2 = m*m;
    return m2*m2*m;
}

// GTR1 (disney.h:56-62).  `a` is a material constant (the clearcoat alpha), so a*a and logf(a*a)
// are evaluated once on the host -- by glibc's logf, i.e. exactly the oracle's value.
TN_D float gtr1(float NDotH, float a, float a2, float logA2)
{
    if (a >= 1) return kInvPi;
    float t = 1 + (a2 - 1)*NDotH*NDotH;
    return (a2 - 1)/(kPi*logA2*t);
}

TN_D float gtr2(float NDotH, float a)      // disney.h:64-69
{
    float a2 = a*a;
    float t = 1.0f + (a2 - 1.0f)*NDotH*NDotH;
    return a2/(kPi*t*t);
}

TN_D float smith_ggx(float NDotv, float alphaG)    // disney.h:71-76
{
    float a = alphaG*alphaG;
    float b = NDotv*NDotv;
    return rcpf_cr(NDotv + sqrtf_cr(a + b - a*b));
}

// etaI/etaT as Fr and BSDFSample take it.  The tolerance build divides by multiplying with v_rcp_f32, and 1.5f*rcp(1.5f) is 1 + 2^-23, not 1: an
// interface between EQUAL indices (a surface met inside a medium of its own index) became one with a critical angle -- SinThetaT2 > 1 below
// VDotN = 5e-4, so F = 1 and a finite pdf where the reference computes 0/0 and drops the sample (VDotN == 0), and Refract() refused the straight
// line.  Found by tests/test_gpu_fast_leaf.py's edge rows; equal indices have the ratio 1 in this build too.
#if TN_FAST
TN_D float index_ratio(float a, float b) { return a == b ? 1.0f : a/b; }
#else
TN_D float index_ratio(float a, float b) { return a/b; }
#endif

TN_D float fresnel_dielectric(float VDotN, float etaI, float etaT)     // Fr, disney.h:79-96
{
    float SinThetaT2 = sqr(index_ratio(etaI, etaT))*(1.0f - VDotN*VDotN);
    if (SinThetaT2 > 1.0f)
        return 1.0f;
    float LDotN = sqrtf_cr(1.0f - SinThetaT2);
    float eta = index_ratio(etaT, etaI);
    float r1 = (VDotN - eta*LDotN)/(VDotN + eta*LDotN);
    float r2 = (LDotN - eta*VDotN)/(LDotN + eta*VDotN);
    return 0.5f*(sqr(r1) + sqr(r2));
}

// BSDFPdf (disney.h:125-166)
TN_D float bsdf_pdf(const Mat& mat, float etaI, float etaO, V3 n, V3 V, V3 L)
{
    if (dot(L, n) <= 0.0f)
    {
        float bsdfPdf = 0.0f;
        float brdfPdf = kInv2Pi*mat.subsurface*0.5f;
        return lerpf(brdfPdf, bsdfPdf, mat.transmission);
    }
    else
    {
        // F only enters through Lerp(brdfPdf, pdfSpec*F, transmission): with transmission == 0 that is brdfPdf + (finite)*0 == brdfPdf for any
        // FINITE F, so opaque materials skip the Fresnel term -- where it is finite.  Fr() divides by VDotN + eta*LDotN and LDotN + eta*VDotN
        // (disney.h:79-96): with a face-forwarded normal VDotN >= 0, and both are > 0 unless VDotN is not: at VDotN == 0 with etaI == etaO the
        // reference computes 0/0, its pdf is NaN and the light sample is dropped (`bsdfPdf > 0` is false).  One path in 5.3e8 of veach 4K meets a
        // light sphere that exactly (round 6, found by the whole frame at 64 spp: tests/test_gpu_configs.py); so: the shortcut only where VDotN > 0.
        const float VDotN = dot(n, V);
        float F = (mat.transmission != 0.0f || !(VDotN > 0.0f)) ? fresnel_dielectric(VDotN, etaI, etaO) : 1.0f;
        const float a = maxT(0.001f, mat.roughness);
        const V3 half = safe_normalize(L + V, V3(0.0f));
        const float cosThetaHalf = absf(dot(half, n));
        const float pdfHalf = gtr2(cosThetaHalf, a)*cosThetaHalf;
        float pdfSpec = 0.25f*pdfHalf/maxT(1.e-6f, dot(L, half));
        float pdfDiff = absf(dot(L, n))*kInvPi*(1.0f - mat.subsurface);
        float bsdfPdf = pdfSpec*F;
        float brdfPdf = lerpf(pdfDiff, pdfSpec, 0.5f);
        return lerpf(brdfPdf, bsdfPdf, mat.transmission);
    }
}

// the GTR2 half-vector sampling shared by both specular branches (disney.h:184-204 == 265-285);
// sin/cos of phiHalf = r1*k2Pi are passed in
TN_D V3 sample_ggx_reflection(const Mat& mat, V3 U, V3 Vt, V3 N, V3 view, float sinPhiHalf, float cosPhiHalf, float r2)
{
    const float a = maxT(0.001f, mat.roughness);
    const float cosThetaHalf = sqrtf_cr((1.0f - r2)/(1.0f + (sqr(a) - 1.0f)*r2));
    const float sinThetaHalf = sqrtf_cr(maxT(0.0f, 1.0f - sqr(cosThetaHalf)));

    V3 half = U*(sinThetaHalf*cosPhiHalf) + Vt*(sinThetaHalf*sinPhiHalf) + N*cosThetaHalf;
    if (dot(half, view) <= 0.0f)
        half = half*(-1.0f);

    return 2.0f*dot(view, half)*half - view;
}

// BSDFSample (disney.h:170-293).  Same random-number draws in the same order and the same
// arithmetic; the three lobe samplers are each written ONCE after the lobe choice so that lanes
// which picked the same lobe through different branches (GGX via the Fresnel branch or via the
// 50/50 BRDF branch) execute it together.
// SLIM (k_bounce's FIT instances, tn_fused.h): mat.transmission and mat.subsurface are +0.0f, so neither `randf() < transmission` nor
// `randf() < subsurface` holds for any draw -- the draws stay (the stream's order), the refraction and the inside lobe go, and `type`
// is kReflected whatever the lobe.
template <bool SLIM = false>
TN_D void bsdf_sample(const Mat& mat, float etaI, float etaO, V3 U, V3 Vt, V3 N, V3 view, V3& light, float& pdf, int& type, Rng& rng)
{
    enum { kLobeGgx, kLobeCosine, kLobeInside };
    int lobe = kLobeGgx;
    float r1, r2;

    const float uTransmission = rng.randf();
    if (!SLIM && uTransmission < mat.transmission)
    {
        float F = fresnel_dielectric(dot(N, view), etaI, etaO);
        if (rng.randf() < F)
        {
            r1 = rng.randf();
            r2 = rng.randf();
            lobe = kLobeGgx;                    // disney.h:180-205
        }
        else
        {
            float eta = index_ratio(etaI, etaO);
            if (refract(view, N, eta, light))   // disney.h:209-219
            {
                type = kSpecular;
                pdf = (1.0f - F)*mat.transmission;
            }
            else
            {
                pdf = 0.0f;
            }
            return;
        }
    }
    else
    {
        r1 = rng.randf();
        r2 = rng.randf();
        if (rng.randf() < 0.5f)
        {
            const float uSubsurface = rng.randf();
            lobe = (!SLIM && uSubsurface < mat.subsurface) ? kLobeInside : kLobeCosine;     // disney.h:243-261
        }
        else
            lobe = kLobeGgx;                                                         // disney.h:264-287
    }

    // every lobe takes sin/cos of ONE angle: GGX phiHalf = r1*k2Pi (disney.h:185), cosine-hemisphere
    // theta = k2Pi*u2 (maths.h:1307), inside-hemisphere phi = k2Pi*Randf (maths.h:1297, after its z draw)
    float zIn = 0.0f;
    float angle;
    if (!SLIM && lobe == kLobeInside)
    {
        zIn = rng.randf();
        angle = k2Pi*rng.randf();
    }
    else
    {
        angle = (lobe == kLobeGgx) ? r1*k2Pi : k2Pi*r2;
    }
    float sn, cs;
    m_sincosf(angle, sn, cs);

    if (lobe == kLobeGgx)
    {
        light = sample_ggx_reflection(mat, U, Vt, N, view, sn, cs, r2);
        type = kReflected;
    }
    else if (SLIM || lobe == kLobeCosine)
    {
        // CosineSampleHemisphere (maths.h:1304-1310, 1319-1325)
        const float r = sqrtf_cr(r1);
        const float sx = r*cs;
        const float sy = r*sn;
        const float z = sqrtf_cr(maxT(0.0f, 1.0f - sx*sx - sy*sy));
        light = U*sx + Vt*sy + N*z;
        type = kReflected;
    }
    else
    {
        // UniformSampleHemisphere (maths.h:1291-1302), z negated to sample inside the surface
        const float w = sqrtf_cr(1.0f - zIn*zIn);
        const float x = cs*w;
        const float y = sn*w;
        light = U*x + Vt*y - N*zIn;
        type = kTransmitted;
    }

    pdf = bsdf_pdf(mat, etaI, etaO, N, view, light);
}

// BSDFEval (disney.h:296-405)
TN_D V3 bsdf_eval(const Mat& mat, float etaI, float etaO, V3 N, V3 V, V3 L)
{
    float NDotL = dot(N, L);
    float NDotV = dot(N, V);

    V3 H = normalize(L + V);

    float NDotH = dot(N, H);
    float LDotH = dot(L, H);

    V3 Cdlin = mat.color;
    V3 Cspec0 = mat.cspec0;

    V3 bsdf(0.0f);
    V3 brdf(0.0f);

    if (mat.transmission > 0.0f)
    {
        if (NDotL <= 0)
        {
            float F = fresnel_dielectric(NDotV, etaI, etaO);
            bsdf = V3(mat.transmission*(1.0f - F)/absf(NDotL)*(1.0f - mat.metallic));
        }
        else
        {
            float a = maxT(0.001f, mat.roughness);
            float Ds = gtr2(NDotH, a);
            float FH = fresnel_dielectric(LDotH, etaI, etaO);
            V3 Fs = lerp3(Cspec0, V3(1.0f), FH);
            float roughg = a;
            float Gs = smith_ggx(NDotV, roughg)*smith_ggx(NDotL, roughg);
            bsdf = Gs*Fs*Ds;
        }
    }

    if (mat.transmission < 1.0f)
    {
        if (NDotL <= 0)
        {
            if (mat.subsurface > 0.0f)
            {
                V3 s = mat.sqrtColor;
                float FL = schlick_fresnel(absf(NDotL)), FV = schlick_fresnel(NDotV);
                float Fd = (1.0f - 0.5f*FL)*(1.0f - 0.5f*FV);
                brdf = kInvPi*s*mat.subsurface*Fd*(1.0f - mat.metallic);
            }
        }
        else
        {
            float a = maxT(0.001f, mat.roughness);
            float Ds = gtr2(NDotH, a);
            float FH = schlick_fresnel(LDotH);
            V3 Fs = lerp3(Cspec0, V3(1.0f), FH);
            float roughg = a;
            float Gs = smith_ggx(NDotV, roughg)*smith_ggx(NDotL, roughg);

            float FL = schlick_fresnel(NDotL), FV = schlick_fresnel(NDotV);
            float Fd90 = 0.5f + 2.0f*LDotH*LDotH*mat.roughness;
            float Fd = lerpf(1.0f, Fd90, FL)*lerpf(1.0f, Fd90, FV);

            // clearcoat == 0: the lobe is 0*Gr*Fc*Dr with Gr, Fc, Dr finite here (NDotL > 0), i.e. +V3(0)
            float coat = 0.0f;
            if (mat.clearcoat != 0.0f)
            {
                float Dr = gtr1(NDotH, mat.clearcoatAlpha, mat.clearcoatA2, mat.clearcoatLogA2);
                float Fc = lerpf(.04f, 1.0f, FH);
                float Gr = smith_ggx(NDotL, .25f)*smith_ggx(NDotV, .25f);
                coat = mat.clearcoat*Gr*Fc*Dr;
            }

            brdf = kInvPi*Fd*Cdlin*(1.0f - mat.metallic)*(1.0f - mat.subsurface) + Gs*Fs*Ds + V3(coat);
        }
    }

    return lerp3(brdf, bsdf, mat.transmission);
}

} // namespace tn

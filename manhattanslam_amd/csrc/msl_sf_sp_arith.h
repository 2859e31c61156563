// msl_sf_sp_arith.h -- the float / double mixtures of the superpixel kernels (msl_sf_sp_assign.hip, msl_sf_sp_seeds.hip) on plain values, in the
// cheapest form that still has the reference's bits.  No memory access, no HIP type: the kernels hand in what they hold, and a host program calls the
// same text (tests/sp_arith_host.cpp checks every identity below bit for bit against the literal expression).
// The library is built with -ffp-contract=off: every fused multiply-add here is written out.
#pragma once

#if defined(__HIPCC__)
#define MSL_SPA_HD __host__ __device__ __forceinline__
#else
#define MSL_SPA_HD inline
#endif

namespace msl {
namespace sf {

constexpr float sp_float_below(float f) { return __builtin_bit_cast(float, __builtin_bit_cast(unsigned, f) - 1u); }   // (positive finite f)
constexpr float sp_float_above(float f) { return __builtin_bit_cast(float, __builtin_bit_cast(unsigned, f) + 1u); }

// Comparisons of a FLOAT x with the reference's DOUBLE constant 0.01 (C++ evaluates (double)x OP 0.01).  0.01 is not a float, and the float nearest
// to it, (float)0.01, is the float next BELOW it (asserted), so there is no float in ((float)0.01, 0.01]:
//   (double)x <  0.01  <=>  x <= 0.01f        (double)x >  -0.01  <=>  x >= -0.01f        (double)x > 0.01  <=>  x > 0.01f
// (NaN: false on both sides.)  One v_cmp_f32 instead of v_cvt_f64_f32 + v_cmp_f64 per test.  The mirror case of the constants whose float lies
// above them (0.4, 0.1, 0.05 in msl_sf_sp_dev.h, and 0.2 here: x < 0.2  <=>  x < 0.2f).
constexpr float SP_001_F = (float)0.01, SP_02_F = (float)0.2;
static_assert((double)SP_001_F < 0.01 && (double)sp_float_above(SP_001_F) > 0.01, "0.01f is the float next below 0.01");
static_assert((double)SP_02_F > 0.2 && (double)sp_float_below(SP_02_F) < 0.2, "0.2f is the float next above 0.2");
MSL_SPA_HD bool sp_lt_001(float x) { return x <= SP_001_F; }         // (double)x < 0.01
MSL_SPA_HD bool sp_gt_001(float x) { return x > SP_001_F; }          // (double)x > 0.01
MSL_SPA_HD bool sp_gt_neg001(float x) { return x >= -SP_001_F; }     // (double)x > -0.01
MSL_SPA_HD bool sp_lt_02(float x) { return x < SP_02_F; }            // (double)x < 0.2

// Correctly rounded (double)p / 100.0 for a FLOAT p >= 0 (finite), without the ~35-instruction f64 divide: q0 = p * RN(1/100), then ONE Markstein
// correction step.  For an arbitrary double two steps are needed (the first only makes the quotient faithful); a float has 29 zero bits at the end
// of its binary64 significand, and for every one of the 2 139 095 040 finite non-negative floats the first step already lands on RN(p / 100)
// (checked exhaustively: tests/sp_arith_host.cpp --all; q0 alone is wrong for 287 M of them).  The contract is in the argument type: kb_assign only
// ever divides the float product intensityDiff * intensityDiff.
MSL_SPA_HD double sp_div100_of_float(float p) {
    const double x = (double)p, y = 0.01;        // RN(1/100)
    const double q0 = x * y;
    return __builtin_fma(__builtin_fma(-q0, 100.0, x), y, q0);
}
// the two-step form, for any finite double x >= 0 (Markstein's theorem; 100 = 1.5625 * 2^6 is not an all-ones significand)
MSL_SPA_HD double sp_div100_of_double(double x) {
    const double y = 0.01;
    const double q0 = x * y;
    const double q1 = __builtin_fma(__builtin_fma(-q0, 100.0, x), y, q0);
    return __builtin_fma(__builtin_fma(-q1, 100.0, x), y, q1);
}

// calculateCost's intensity term (src/SurfelFusion.cpp:341): nodepthCost += intensityDiff * intensityDiff / 100.0, the float product divided in double
MSL_SPA_HD float sp_cost_add_intensity(float nodepthCost, float intensityDiff) {
    return (float)((double)nodepthCost + sp_div100_of_float(intensityDiff * intensityDiff));
}
// ... and its depth term (:350): (float)((double)nodepthCost + (double)(d * d) * 400.0).  A float times 400.0 needs 24 + 9 significand bits: the product
// is exact in binary64, so the fused form rounds once, at the same place, to the same bits.
MSL_SPA_HD float sp_cost_add_depth(float nodepthCost, float inverseDepthDiff) {
    return (float)__builtin_fma((double)(inverseDepthDiff * inverseDepthDiff), 400.0, (double)nodepthCost);
}

// The Newton step of updateSeeds (:505): deltaDepth = (float)((double)(-sumA) / ((double)sumB + 10.0)) with sumB = (float)(2 * inr), inr <= 256 in-band
// depths.  The denominator is an even integer in [10, 522]: exactly a float, and both operands of the binary64 division are float values.  Rounding
// the binary64 quotient of two floats to float is the correctly rounded float quotient (double rounding is innocuous for division when 53 >= 2 * 24
// + 2), so the IEEE float division has the same bits -- for NaN and infinite numerators too (compared on the device by msl_debug_sp_arith).
constexpr int SP_NEWTON_MAX_INR = 256;
MSL_SPA_HD float sp_newton_delta(float sumA, int inr) {
    const float sumB = (float)(2 * inr);
    return (-sumA) / (sumB + 10.0f);
}
// the literal expression (the test hook and the host program compare against it)
MSL_SPA_HD float sp_newton_delta_literal(float sumA, int inr) {
    const float sumB = (float)(2 * inr);
    return (float)((double)(-sumA) / ((double)sumB + 10.0));
}

// ---- FP64 sums over the 16 lanes of a seed group (kb_seed_plane), several values at once ------------------------------------------------------
// The butterfly sums ONE value over the 16 lanes of a DPP row, every lane receiving the total: s1[i] = v[i] + v[i - 8], s2[i] = s1[i] + s1[i - 4],
// s3[i] = s2[i] + s2[i ^ 2], s4[i] = s3[i] + s3[i ^ 1] (lane numbers mod 16; three instructions per step: two DPP moves and the add).  Its readers
// need far less: the Gauss-Newton update reads J_a in lanes 4 a .. 4 a + 3 only, and each Hessian entry is stored by one lane.  So several values are
// reduced jointly, TRANSPOSED: at the ror:8 step a lane keeps the value its bit 3 selects and hands the other one over, at the ror:4 step the same by
// bit 2; the quad steps finish.  Every partial sum has the two operands the butterfly gives it in that lane (s1 and s2 do not depend on the lane bits
// already folded, by commutativity), and FP addition is commutative, so every total has the butterfly's bits.
// The schedule is written on a lane-vector type V with the operations of Ops, so that a host program runs the same text on arrays of 16 doubles:
//   Ops::sel<CTRL, BANKS>(old, src)   DPP move with control CTRL into the banks (lanes 4 k .. 4 k + 3 <-> bit k) of BANKS, `old` elsewhere
//   Ops::mov<CTRL>(v)                 DPP move into every lane
//   Ops::add(a, b)                    a + b per lane
constexpr int SP_ROR4 = 0x124, SP_ROR8 = 0x128, SP_ROR12 = 0x12C, SP_QUAD_2301 = 0x4E, SP_QUAD_1032 = 0xB1;   // row_ror:n hands lane i the value of lane i - n (mod 16)
// lanes 0-7: x[i] + x[i + 8], lanes 8-15: y[i - 8] + y[i]
template <class Ops, class V> MSL_SPA_HD V sp_fold8(V x, V y) { return Ops::add(Ops::template sel<SP_ROR8, 0xC>(x, y), Ops::template sel<SP_ROR8, 0x3>(y, x)); }
// banks 0, 2: a[i] + a[i + 4], banks 1, 3: b[i - 4] + b[i]
template <class Ops, class V> MSL_SPA_HD V sp_fold4(V a, V b) { return Ops::add(Ops::template sel<SP_ROR4, 0xA>(a, b), Ops::template sel<SP_ROR12, 0x5>(b, a)); }
template <class Ops, class V> MSL_SPA_HD V sp_quad_sum(V v) {
    v = Ops::add(v, Ops::template mov<SP_QUAD_2301>(v));
    return Ops::add(v, Ops::template mov<SP_QUAD_1032>(v));
}
// the butterfly itself (one value, the total in every lane)
template <class Ops, class V> MSL_SPA_HD V sp_group_sum(V v) {
    v = Ops::add(v, Ops::template mov<SP_ROR8>(v));
    v = Ops::add(v, Ops::template mov<SP_ROR4>(v));
    return sp_quad_sum<Ops>(v);
}
// Four values: lane 4 a + b receives the total of v_a.
template <class Ops, class V> MSL_SPA_HD V sp_group_sum4(V v0, V v1, V v2, V v3) {
    return sp_quad_sum<Ops>(sp_fold4<Ops>(sp_fold8<Ops>(v0, v2), sp_fold8<Ops>(v1, v3)));
}
// The ten sums of the symmetric 4x4 Hessian as three lane vectors:
//   c0: bank a holds H0a        c1: banks 0 .. 3 hold H11, H12, H13, H22        c2: bank 1 holds H23, bank 3 holds H33 (banks 0, 2: nothing)
template <class V> struct SpHessSums { V c0, c1, c2; };
template <class Ops, class V> MSL_SPA_HD SpHessSums<V> sp_group_sum10(V h00, V h01, V h02, V h03, V h11, V h12, V h13, V h22, V h23, V h33) {
    SpHessSums<V> r;
    r.c0 = sp_quad_sum<Ops>(sp_fold4<Ops>(sp_fold8<Ops>(h00, h02), sp_fold8<Ops>(h01, h03)));
    r.c1 = sp_quad_sum<Ops>(sp_fold4<Ops>(sp_fold8<Ops>(h11, h13), sp_fold8<Ops>(h12, h22)));
    const V a2 = sp_fold8<Ops>(h23, h33);   // lanes 0-7: H23, lanes 8-15: H33; the plain ror:4 step is then right where lane i - 4 holds the same value
    r.c2 = sp_quad_sum<Ops>(Ops::add(a2, Ops::template mov<SP_ROR4>(a2)));
    return r;
}
// Lane l of the group stores what it holds of the Hessian + 5 I (column-major, both triangles) into m[16]: the first lane of each bank.
MSL_SPA_HD void sp_hessian_store(double *m, int l, double c0, double c1, double c2) {
    if (l & 3) return;
    const int a = l >> 2;
    const double d0 = a == 0 ? c0 + 5 : c0;                  // H00 + 5 | H01 | H02 | H03
    m[a] = d0; m[4 * a] = d0;
    const double d1 = (a == 0 || a == 3) ? c1 + 5 : c1;      // H11 + 5 | H12 | H13 | H22 + 5
    m[(0xA765u >> (4 * a)) & 15u] = d1; m[(0xAD95u >> (4 * a)) & 15u] = d1;   // 5, 5 | 6, 9 | 7, 13 | 10, 10
    if (a & 1) {
        const double d2 = a == 3 ? c2 + 5 : c2;              // H23 | H33 + 5
        m[a == 1 ? 11 : 15] = d2; m[a == 1 ? 14 : 15] = d2;
    }
}

}  // namespace sf
}  // namespace msl

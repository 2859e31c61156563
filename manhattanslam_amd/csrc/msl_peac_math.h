// msl_peac_math.h -- the FP64 arithmetic the plane extractor's device kernels (msl_peac.hip) and its host stage (msl_peac_host.hip) share, so
// both sides produce the same bits: the 3x3 symmetric eigen-solver, the PCA plane fit built on it, and the cloud vertex of a depth pixel (internal).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/msl.h"

namespace msl {
namespace peac {

// ---- arithmetic shared by the device kernel and the host clustering (same expressions, IEEE double, no FMA contraction) ----
__host__ __device__ inline double hypot_pos(double x, double y) {   // Eigen::numext::hypot
    const double ax = fabs(x), ay = fabs(y);
    double p, qp;
    if (ax > ay) { p = ax; qp = ay / p; } else { p = ay; qp = ax / p; }
    if (p == 0) return 0;
    return p * sqrt(1.0 + qp * qp);
}

// Eigen::SelfAdjointEigenSolver<Matrix3d>::compute as LA::eig33sym uses it: s[0] <= s[1] <= s[2], V[:][i] the eigenvector of s[i].
// (lower triangle scaled by its largest coefficient, closed-form 3x3 Householder tridiagonalisation, implicit symmetric QR with
// Wilkinson shift and the 2-epsilon deflation test, eigenvalues sorted increasingly with their vectors)
// VECTORS = false leaves out the accumulation of the rotations (q never feeds back into the diagonal / sub-diagonal updates, so the eigenvalues are the
// same bits either way): the clustering only needs the smallest eigenvalue of every candidate merge and the vectors of the one it accepts.
// The diagonal, the sub-diagonal and the rotation matrix are named scalars and every "array" access with a run-time index is a select: the device
// kernels keep them in registers (round 5: the indexed local arrays of rounds 1-4 lived in 80 bytes of scratch memory per lane).  Same operations in
// the same order as before, so the same bits (tests/test_peac_host.py compares against the oracle and the SIMD-lane form).
template <bool VECTORS>
__host__ __device__ inline void eig33sym_t(const double K[3][3], double s[3], double V[3][3]) {
    double a00 = K[0][0], a10 = K[1][0], a11 = K[1][1], a20 = K[2][0], a21 = K[2][1], a22 = K[2][2];
    double scale = fmax(fmax(fmax(fabs(a00), fabs(a10)), fmax(fabs(a11), fabs(a20))), fmax(fabs(a21), fabs(a22)));
    if (scale == 0) scale = 1;
    a00 /= scale; a10 /= scale; a11 /= scale; a20 /= scale; a21 /= scale; a22 /= scale;
    double d0 = a00, d1, d2, e0, e1;
    double q00 = 1, q01 = 0, q02 = 0, q10 = 0, q11 = 1, q12 = 0, q20 = 0, q21 = 0, q22 = 1;
    const double tiny = 2.2250738585072014e-308;   // std::numeric_limits<double>::min()
    const double v1norm2 = a20 * a20;
    if (v1norm2 <= tiny) {
        d1 = a11; d2 = a22; e0 = a10; e1 = a21;
    } else {
        const double beta = sqrt(a10 * a10 + v1norm2);
        const double invBeta = 1.0 / beta;
        const double m01 = a10 * invBeta, m02 = a20 * invBeta;
        const double qq = 2.0 * m01 * a21 + m02 * (a22 - a11);
        d1 = a11 + m02 * qq; d2 = a22 - m02 * qq;
        e0 = beta; e1 = a21 - m01 * qq;
        if (VECTORS) { q11 = m01; q12 = m02; q21 = m02; q22 = -m01; }
    }
    // dg[i] = (d0, d1, d2)[i], sb[i] = (e0, e1)[i]
    auto DG = [&](int i) -> double { return i == 0 ? d0 : (i == 1 ? d1 : d2); };
    auto SB = [&](int i) -> double { return i == 0 ? e0 : e1; };
    auto setDG = [&](int i, double v) { if (i == 0) d0 = v; else if (i == 1) d1 = v; else d2 = v; };
    auto setSB = [&](int i, double v) { if (i == 0) e0 = v; else e1 = v; };
    int end = 2, start = 0, iter = 0;
    const double precision = 2.0 * 2.220446049250313e-16;
    while (end > 0) {
        for (int i = start; i < end; ++i)
            if (fabs(SB(i)) <= (fabs(DG(i)) + fabs(DG(i + 1))) * precision || fabs(SB(i)) <= tiny) setSB(i, 0);
        while (end > 0 && SB(end - 1) == 0.0) end--;
        if (end <= 0) break;
        if (++iter > 30 * 3) break;
        start = end - 1;
        while (start > 0 && SB(start - 1) != 0) start--;
        const double td = (DG(end - 1) - DG(end)) * 0.5, e = SB(end - 1);
        double mu = DG(end);
        if (td == 0.0) mu -= fabs(e);
        else if (e != 0.0) {
            const double e2 = e * e, h = hypot_pos(td, e);
            if (e2 == 0.0) mu -= e / ((td + (td > 0.0 ? h : -h)) / e);
            else mu -= e2 / (td + (td > 0.0 ? h : -h));
        }
        double x = DG(start) - mu, z = SB(start);
        for (int k = start; k < end && z != 0.0; ++k) {
            double c, sn;   // Givens rotation that annihilates z against x
            if (x == 0.0) { c = 0.0; sn = z < 0.0 ? 1.0 : -1.0; }
            else if (fabs(x) > fabs(z)) { const double t = z / x; double u = sqrt(1.0 + t * t); if (x < 0.0) u = -u; c = 1.0 / u; sn = -t * c; }
            else { const double t = x / z; double u = sqrt(1.0 + t * t); if (z < 0.0) u = -u; sn = -1.0 / u; c = -t * sn; }
            const double dk = DG(k), dk1 = DG(k + 1), sk = SB(k);
            const double sdk = sn * dk + c * sk;
            const double dkp1 = sn * sk + c * dk1;
            setDG(k, c * (c * dk - sn * sk) - sn * (c * sk - sn * dk1));
            setDG(k + 1, sn * sdk + c * dkp1);
            const double skNew = c * sdk - sn * dkp1;
            setSB(k, skNew);
            if (k > start) setSB(k - 1, c * SB(k - 1) - sn * z);
            x = skNew;
            if (k < end - 1) { const double s1 = SB(k + 1); z = -sn * s1; setSB(k + 1, c * s1); }
            if (VECTORS) {   // columns k, k + 1 of q (k is 0 or 1)
                if (k == 0) {
                    const double x0 = q00, y0 = q01, x1 = q10, y1 = q11, x2 = q20, y2 = q21;
                    q00 = c * x0 - sn * y0; q01 = sn * x0 + c * y0;
                    q10 = c * x1 - sn * y1; q11 = sn * x1 + c * y1;
                    q20 = c * x2 - sn * y2; q21 = sn * x2 + c * y2;
                } else {
                    const double x0 = q01, y0 = q02, x1 = q11, y1 = q12, x2 = q21, y2 = q22;
                    q01 = c * x0 - sn * y0; q02 = sn * x0 + c * y0;
                    q11 = c * x1 - sn * y1; q12 = sn * x1 + c * y1;
                    q21 = c * x2 - sn * y2; q22 = sn * x2 + c * y2;
                }
            }
        }
    }
    // selection sort, columns follow: i = 0 picks the smallest of (d0, d1, d2), i = 1 the smaller of the remaining two
    {
        int k = 0;
        if (d1 < d0) k = 1;
        if (d2 < (k == 0 ? d0 : d1)) k = 2;
        if (k == 1) {
            const double t = d0; d0 = d1; d1 = t;
            if (VECTORS) { double u = q00; q00 = q01; q01 = u; u = q10; q10 = q11; q11 = u; u = q20; q20 = q21; q21 = u; }
        } else if (k == 2) {
            const double t = d0; d0 = d2; d2 = t;
            if (VECTORS) { double u = q00; q00 = q02; q02 = u; u = q10; q10 = q12; q12 = u; u = q20; q20 = q22; q22 = u; }
        }
        if (d2 < d1) {
            const double t = d1; d1 = d2; d2 = t;
            if (VECTORS) { double u = q01; q01 = q02; q02 = u; u = q11; q11 = q12; q12 = u; u = q21; q21 = q22; q22 = u; }
        }
    }
    s[0] = d0 * scale; s[1] = d1 * scale; s[2] = d2 * scale;
    if (VECTORS) { V[0][0] = q00; V[0][1] = q01; V[0][2] = q02; V[1][0] = q10; V[1][1] = q11; V[1][2] = q12; V[2][0] = q20; V[2][1] = q21; V[2][2] = q22; }
}
__host__ __device__ inline void eig33sym(const double K[3][3], double s[3], double V[3][3]) { eig33sym_t<true>(K, s, V); }

// ahc::PlaneSeg::Stats::compute (AHCPlaneSeg.hpp:148-183)
__host__ __device__ inline void plane_fit(const msl_peac_stats &st, double center[3], double normal[3], double &mse, double &curvature) {
    const double sc = ((double)1.0) / st.N;
    center[0] = st.sx * sc; center[1] = st.sy * sc; center[2] = st.sz * sc;
    double K[3][3] = {{st.sxx - st.sx * st.sx * sc, st.sxy - st.sx * st.sy * sc, st.sxz - st.sx * st.sz * sc},
                      {0, st.syy - st.sy * st.sy * sc, st.syz - st.sy * st.sz * sc},
                      {0, 0, st.szz - st.sz * st.sz * sc}};
    K[1][0] = K[0][1]; K[2][0] = K[0][2]; K[2][1] = K[1][2];
    double sv[3], V[3][3];
    eig33sym(K, sv, V);
    const double sgn = (V[0][0] * center[0] + V[1][0] * center[1] + V[2][0] * center[2] <= 0) ? 1.0 : -1.0;   // normal towards the camera
    normal[0] = sgn > 0 ? V[0][0] : -V[0][0]; normal[1] = sgn > 0 ? V[1][0] : -V[1][0]; normal[2] = sgn > 0 ? V[2][0] : -V[2][0];
    mse = sv[0] * sc;
    curvature = sv[0] / (sv[0] + sv[1] + sv[2]);
}

// the MSE plane_fit would report, without centre / normal / curvature (the same K, the same eigenvalue bits)
__host__ __device__ inline double plane_mse(const msl_peac_stats &st) {
    const double sc = ((double)1.0) / st.N;
    double K[3][3] = {{st.sxx - st.sx * st.sx * sc, st.sxy - st.sx * st.sy * sc, st.sxz - st.sx * st.sz * sc},
                      {0, st.syy - st.sy * st.sy * sc, st.syz - st.sy * st.sz * sc},
                      {0, 0, st.szz - st.sz * st.sz * sc}};
    K[1][0] = K[0][1]; K[2][0] = K[0][2]; K[2][1] = K[1][2];
    double sv[3];
    eig33sym_t<false>(K, sv, nullptr);
    return sv[0] * sc;
}

// z of cloud vertex (row, col): (double)depth(2 row, 2 col) * depthMapFactor (src/PlaneExtractor.cpp:64)
__host__ __device__ inline double vertex_z(const uint16_t *img, size_t strideBytes, float factor, int row, int col) {
    const uint16_t d = *reinterpret_cast<const uint16_t *>(reinterpret_cast<const uint8_t *>(img) + (size_t)(2 * row) * strideBytes + 2 * (size_t)(2 * col));
    return (double)d * factor;
}
__host__ __device__ inline void vertex_xy(float fx, float fy, float cx, float cy, int row, int col, double z, double &x, double &y) {
    x = ((double)(2 * col) - cx) * z / fx;   // :69
    y = ((double)(2 * row) - cy) * z / fy;   // :70
}

}  // namespace peac
}  // namespace msl

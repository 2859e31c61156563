// msl_pnp.hip -- batched EPnP RANSAC for gfx950: PnPsolver (reference src/PnPsolver.cc) as Tracking::Relocalization uses it
// (src/Tracking.cc:1960-2000): msl_pnp_ransac[_batch] = n_pairs independent runs of one iterate() call on a fresh solver.
//
// Kernels (one wave per workgroup; every matrix lives in LDS, the correspondences are read in place):
//   k_pnp_gather      one wave per pair: the valid matches compacted in ascending keypoint order (PnPsolver.cc:76-96), N and the iteration count
//   k_pnp_hypothesis  one wave per (pair, iteration): the sample, compute_pose on its four points, CheckInliers over the pair's N
//                     correspondences -> count, bit mask, pose
//   k_pnp_resolve     one wave per pair: walks the records (count >= minInliers and above every earlier count) in iteration order, runs
//                     Refine() = compute_pose over the record's inliers + CheckInliers, stops at the first success, writes the outputs
//
// Pins where the reference is undefined or not restated (tests/pnp_model.py is the sequential model):
//   * sampling: draw j of iteration k = fmix32(fmix32(seed ^ k * 0x9E3779B1) ^ (j + 1) * 0x85EBCA77), randi = mulhi32(hash, available)
//     (msl_match_math.h: sampler_draw)
//   * cvSVD / cvSolve / cvInvert: a cyclic Jacobi method on the symmetric matrix (A^T A for the least-squares solves, the inverse and the
//     3x3 SVD), msl_jacobi.h's schedule and rotation run by the whole wave: round-robin steps of disjoint pairs, the angles of a step from
//     the matrix before it, all row updates, then all column updates; JACOBI_SWEEPS sweeps, no convergence branch; a pair with a_pq == 0
//     is skipped; eigenpairs sorted by descending eigenvalue, the lower index first on ties, no sign normalisation; + - * / sqrt only
//   * every sum over correspondences runs left to right from 0.0 in one lane; the lanes share out the ENTRIES (the 78 of M^T M, the 9 of ABt)
//   * gauss_newton's X starts as zeros (qr_solve's singular early-out leaves it as it was)
#include "msl_jacobi.h"
#include "msl_match_handle.h"
#include "msl_match_math.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace {

using namespace msl;

constexpr int MAX_KCAP = 32768, MAX_ITS = 1024;   // MAX_KCAP: map points a pair may name (msl_reloc.hip has a kcap of its own)
constexpr double PINV_TOL = 1e-12;           // eigenvalues of A^T A at or below PINV_TOL * the largest are dropped by the pseudo-inverse

struct PnpDev {
    int cap, kcap, kmax, words, nIter, nlevels;
    float fx, fy, cx, cy, th2;
    float sigma2[MSL_MATCH_MAX_LEVELS];
    const msl_keypoint *kps; const float *unxy; const int32_t *match; const int32_t *nKps; const float *xyz; const uint32_t *seed;
    const int32_t *table;                                      // [cap + 1][2]: N -> (minInliers, maxIts)
    float *p2d, *p3d, *maxErr; int32_t *kpIdx, *N, *Kit;       // the compacted correspondences [pairs][cap]; per pair N and the iterations run
    unsigned long long *mask; int32_t *count; double *hypRt; int32_t *hypBranch;   // per hypothesis [pairs][kmax]
    int32_t *ridx; unsigned long long *rmask;                  // Refine(): its correspondences [pairs][cap], its inlier mask [pairs][words]
    float *Tcw; uint8_t *inlier; int32_t *ptRef, *nInl, *status;
};

// One set of correspondences: list[i] indexes the pair's compacted arrays.
struct Corr {
    const float *p3d, *p2d; const int32_t *list; int n;
    __device__ void load(int i, double pw[3], double u[2]) const {
        const int j = list[i];
        pw[0] = (double)p3d[3 * j]; pw[1] = (double)p3d[3 * j + 1]; pw[2] = (double)p3d[3 * j + 2];
        u[0] = (double)p2d[2 * j]; u[1] = (double)p2d[2 * j + 1];
    }
};

// The wave's LDS.
struct Work {
    double A[144], V[144];                  // the Jacobi iterate and its eigenvectors (columns)
    double ut[144];                         // compute_pose's Ut (rows = eigenvectors of M^T M, descending)
    double uts[25], ds[12];                 // the latest eigen-solve's sorted eigenvector rows (n <= 5) / eigenvalues
    double c[6], s[6]; int jp[6], jq[6], rk[12];
    double cws[4][3], ci[9];
    double L[60], rho[6];
    double S[30], atb[5], y[5], bx[5];      // a 6 x k sub-matrix of L / cc / ABt; the least-squares solve
    double betas[4], ccs[4][3], pc0[3], U[9];
    double ga[24], gb[6], gx[4], gA1[4], gA2[4];
    double R[3][9], t[3][3], err[3];
    double Rf[9], tf[3]; int branch;
    int idx[4];
};

__device__ __forceinline__ double dot3_f64(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// Eigenpairs of the symmetric n x n matrix in W.A (n <= 12): d[n] descending, ut[n][n] with the eigenvectors as rows.  Whole wave.
__device__ __forceinline__ void jacobi(Work &W, int n, double *d, double *ut) {
    const int lane = threadIdx.x;
    for (int e = lane; e < n * n; e += WAVE) W.V[e] = (e / n == e % n) ? 1.0 : 0.0;
    const int steps = jacobi_steps(n), half = jacobi_slots(n);
    __syncthreads();
    for (int sw = 0; sw < JACOBI_SWEEPS; sw++)
        for (int r = 0; r < steps; r++) {
            if (lane < half) {
                const JacobiPair pq = jacobi_pair(n, r, lane);
                int p = pq.p;
                const int q = pq.q;
                if (q < n) {
                    const JacobiRot R = jacobi_rotation(W.A[p * n + p], W.A[q * n + q], W.A[p * n + q]);
                    if (R.skip) p = -1;                                       // a_pq == 0
                    else { W.c[lane] = R.c; W.s[lane] = R.s; }
                } else {
                    p = -1;                                                   // the padding index
                }
                W.jp[lane] = p; W.jq[lane] = q;
            }
            __syncthreads();
            for (int it = lane; it < half * n; it += WAVE) {                 // rows p, q of A
                const int pr = it / n, j = it - pr * n, p = W.jp[pr], q = W.jq[pr];
                if (p >= 0) {
                    const double c = W.c[pr], s = W.s[pr], x = W.A[p * n + j], y = W.A[q * n + j];
                    W.A[p * n + j] = c * x - s * y; W.A[q * n + j] = s * x + c * y;
                }
            }
            __syncthreads();
            for (int it = lane; it < 2 * half * n; it += WAVE) {             // columns p, q of A and of V
                const int w = it / (half * n), r2 = it - w * half * n, pr = r2 / n, i = r2 - pr * n, p = W.jp[pr], q = W.jq[pr];
                if (p >= 0) {
                    double *X = w ? W.V : W.A;
                    const double c = W.c[pr], s = W.s[pr], x = X[i * n + p], y = X[i * n + q];
                    X[i * n + p] = c * x - s * y; X[i * n + q] = s * x + c * y;
                }
            }
            __syncthreads();
        }
    if (lane < n) {
        const double di = W.A[lane * n + lane];
        int rank = 0;
        for (int j = 0; j < n; j++) { const double dj = W.A[j * n + j]; rank += (dj > di || (dj == di && j < lane)) ? 1 : 0; }
        W.rk[lane] = rank; d[rank] = di;
    }
    __syncthreads();
    for (int e = lane; e < n * n; e += WAVE) { const int i = e / n, a = e - i * n; ut[W.rk[i] * n + a] = W.V[a * n + i]; }
    __syncthreads();
}

// W.A = S^T S for the rows x k matrix S (left-to-right sums over the rows); whole wave, no barrier at the end.
__device__ __forceinline__ void gram(Work &W, const double *S, int rows, int k) {
    for (int e = threadIdx.x; e < k * k; e += WAVE) {
        const int a = e / k, b = e - a * k;
        double acc = 0.0;
        for (int r = 0; r < rows; r++) acc = acc + S[r * k + a] * S[r * k + b];
        W.A[e] = acc;
    }
}

__device__ __forceinline__ double inv_eig(const double *d, int j) { return d[j] > d[0] * PINV_TOL ? 1.0 / d[j] : 0.0; }

// cvSolve(S, rho, x, CV_SVD) for the 6 x k matrix W.S: W.bx = V diag(1 / d) V^T S^T rho.  Whole wave.
__device__ __forceinline__ void pinv_solve(Work &W, int k) {
    const int lane = threadIdx.x;
    gram(W, W.S, 6, k);
    __syncthreads();
    jacobi(W, k, W.ds, W.uts);
    if (lane < k) { double acc = 0.0; for (int r = 0; r < 6; r++) acc = acc + W.S[r * k + lane] * W.rho[r]; W.atb[lane] = acc; }
    __syncthreads();
    if (lane < k) { double acc = 0.0; for (int a = 0; a < k; a++) acc = acc + W.uts[lane * k + a] * W.atb[a]; W.y[lane] = acc * inv_eig(W.ds, lane); }
    __syncthreads();
    if (lane < k) { double acc = 0.0; for (int j = 0; j < k; j++) acc = acc + W.uts[j * k + lane] * W.y[j]; W.bx[lane] = acc; }
    __syncthreads();
}

__device__ __forceinline__ void alphas(const Work &W, const double pw[3], double a[4]) {
    const double d0 = pw[0] - W.cws[0][0], d1 = pw[1] - W.cws[0][1], d2 = pw[2] - W.cws[0][2];
    a[1] = W.ci[0] * d0 + W.ci[1] * d1 + W.ci[2] * d2;
    a[2] = W.ci[3] * d0 + W.ci[4] * d1 + W.ci[5] * d2;
    a[3] = W.ci[6] * d0 + W.ci[7] * d1 + W.ci[8] * d2;
    a[0] = 1.0 - a[1] - a[2] - a[3];
}

// Column `col` of fill_M's first (row2 = 0) or second row for one correspondence.
__device__ __forceinline__ double m_entry(int col, int row2, const double a[4], double fu, double fv, double du, double dv) {
    const int j = col / 3, c = col - 3 * j;
    const double aj = j == 0 ? a[0] : j == 1 ? a[1] : j == 2 ? a[2] : a[3];
    if (row2 == 0) return c == 0 ? aj * fu : c == 1 ? 0.0 : aj * du;
    return c == 0 ? 0.0 : c == 1 ? aj * fv : aj * dv;
}

// The file's Householder qr_solve (PnPsolver.cc:803-892) on W.ga (6 x 4) and W.gb -> W.gx; one lane.
__device__ __forceinline__ void qr_solve(Work &W) {
    constexpr int nr = 6, nc = 4;
    double *A = W.ga, *b = W.gb, *X = W.gx;
    for (int k = 0; k < nc; k++) {
        double eta = fabs(A[k * nc + k]);
        for (int i = k; i < nr - 1; i++) { const double elt = fabs(A[i * nc + k]); if (eta < elt) eta = elt; }   // its scan stops one row short
        if (eta == 0) return;                                                                                  // "A is singular": X stays
        const double inv_eta = 1. / eta;
        double sum = 0.0;
        for (int i = k; i < nr; i++) { A[i * nc + k] = A[i * nc + k] * inv_eta; sum = sum + A[i * nc + k] * A[i * nc + k]; }
        double sigma = sqrt(sum);
        if (A[k * nc + k] < 0) sigma = -sigma;
        A[k * nc + k] = A[k * nc + k] + sigma;
        W.gA1[k] = sigma * A[k * nc + k];
        W.gA2[k] = -eta * sigma;
        for (int j = k + 1; j < nc; j++) {
            double s2 = 0;
            for (int i = k; i < nr; i++) s2 = s2 + A[i * nc + k] * A[i * nc + j];
            const double tau = s2 / W.gA1[k];
            for (int i = k; i < nr; i++) A[i * nc + j] = A[i * nc + j] - tau * A[i * nc + k];
        }
    }
    for (int j = 0; j < nc; j++) {
        double tau = 0;
        for (int i = j; i < nr; i++) tau = tau + A[i * nc + j] * b[i];
        tau = tau / W.gA1[j];
        for (int i = j; i < nr; i++) b[i] = b[i] - tau * A[i * nc + j];
    }
    X[nc - 1] = b[nc - 1] / W.gA2[nc - 1];
    for (int i = nc - 2; i >= 0; i--) {
        double sum = 0;
        for (int j = i + 1; j < nc; j++) sum = sum + A[i * nc + j] * X[j];
        X[i] = (b[i] - sum) / W.gA2[i];
    }
}

// gauss_newton (:784-801) on W.betas; one lane.
__device__ __forceinline__ void gauss_newton(Work &W) {
    for (int i = 0; i < 4; i++) W.gx[i] = 0.0;
    for (int it = 0; it < 5; it++) {
        const double b0 = W.betas[0], b1 = W.betas[1], b2 = W.betas[2], b3 = W.betas[3];
        for (int i = 0; i < 6; i++) {
            const double *l = W.L + 10 * i;
            double *a = W.ga + 4 * i;
            a[0] = 2 * l[0] * b0 + l[1] * b1 + l[3] * b2 + l[6] * b3;
            a[1] = l[1] * b0 + 2 * l[2] * b1 + l[4] * b2 + l[7] * b3;
            a[2] = l[3] * b0 + l[4] * b1 + 2 * l[5] * b2 + l[8] * b3;
            a[3] = l[6] * b0 + l[7] * b1 + l[8] * b2 + 2 * l[9] * b3;
            W.gb[i] = W.rho[i] - (l[0] * b0 * b0 + l[1] * b0 * b1 + l[2] * b1 * b1 + l[3] * b0 * b2 + l[4] * b1 * b2 + l[5] * b2 * b2 +
                                  l[6] * b0 * b3 + l[7] * b1 * b3 + l[8] * b2 * b3 + l[9] * b3 * b3);
        }
        qr_solve(W);
        for (int i = 0; i < 4; i++) W.betas[i] = W.betas[i] + W.gx[i];
    }
}

// PnPsolver::compute_pose (:442-489) over the correspondences C: the pose into W.Rf, W.tf, the winning branch into W.branch.  Whole wave.
__device__ __forceinline__ void compute_pose(Work &W, const Corr &C, double fu, double fv, double uc, double vc) {
    const int lane = threadIdx.x, n = C.n;
    const double dn = (double)n;
    double pw[3], u[2], a[4];
    // choose_control_points: the centroid (it is estimate_R_and_t's pw0 as well), PCA
    if (lane < 3) {
        double acc = 0.0;
        for (int i = 0; i < n; i++) { C.load(i, pw, u); acc = acc + (lane == 0 ? pw[0] : lane == 1 ? pw[1] : pw[2]); }
        W.cws[0][lane] = acc / dn;
    }
    __syncthreads();
    if (lane < 9) {
        const int j = lane / 3, k = lane - 3 * j;
        double acc = 0.0;
        for (int i = 0; i < n; i++) {
            C.load(i, pw, u);
            const double x = (j == 0 ? pw[0] : j == 1 ? pw[1] : pw[2]) - W.cws[0][j], y = (k == 0 ? pw[0] : k == 1 ? pw[1] : pw[2]) - W.cws[0][k];
            acc = acc + x * y;
        }
        W.A[lane] = acc;
    }
    __syncthreads();
    jacobi(W, 3, W.ds, W.uts);
    if (lane < 9) {
        const int i = lane / 3, j = lane - 3 * i;
        const double dc = W.ds[i], kk = sqrt((dc > 0 ? dc : 0.0) / dn);
        W.cws[1 + i][j] = W.cws[0][j] + kk * W.uts[lane];
    }
    __syncthreads();
    // compute_barycentric_coordinates: cvInvert(CC, CC_inv, CV_SVD)
    if (lane < 9) { const int i = lane / 3, j = lane - 3 * i; W.S[lane] = W.cws[1 + j][i] - W.cws[0][i]; }
    __syncthreads();
    gram(W, W.S, 3, 3);
    __syncthreads();
    jacobi(W, 3, W.ds, W.uts);
    if (lane < 9) {                                                            // B[j][c] = sum_a V[a][j] CC[c][a], scaled by 1 / d_j
        const int j = lane / 3, c = lane - 3 * j;
        double acc = 0.0;
        for (int q = 0; q < 3; q++) acc = acc + W.uts[j * 3 + q] * W.S[c * 3 + q];
        W.U[lane] = acc * inv_eig(W.ds, j);
    }
    __syncthreads();
    if (lane < 9) {
        const int r = lane / 3, c = lane - 3 * r;
        double acc = 0.0;
        for (int j = 0; j < 3; j++) acc = acc + W.uts[j * 3 + r] * W.U[j * 3 + c];
        W.ci[lane] = acc;
    }
    __syncthreads();
    // M^T M: entry (p, q), p <= q, per lane; the rows of M in order (two per correspondence)
    for (int e = lane; e < 78; e += WAVE) {
        int p = 0, r = e;
        while (r >= 12 - p) { r -= 12 - p; p++; }
        const int q = p + r;
        double acc = 0.0;
        for (int i = 0; i < n; i++) {
            C.load(i, pw, u);
            alphas(W, pw, a);
            const double du = uc - u[0], dv = vc - u[1];
            acc = acc + m_entry(p, 0, a, fu, fv, du, dv) * m_entry(q, 0, a, fu, fv, du, dv);
            acc = acc + m_entry(p, 1, a, fu, fv, du, dv) * m_entry(q, 1, a, fu, fv, du, dv);
        }
        W.A[p * 12 + q] = acc; W.A[q * 12 + p] = acc;
    }
    __syncthreads();
    jacobi(W, 12, W.ds, W.ut);
    // compute_L_6x10, compute_rho
    if (lane < 6) {
        const int pa = lane < 3 ? 0 : lane < 5 ? 1 : 2, pb = lane < 3 ? lane + 1 : lane < 5 ? lane - 1 : 3;
        double dv[4][3];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const double *v = W.ut + 12 * (11 - i);
#pragma unroll
            for (int c = 0; c < 3; c++) dv[i][c] = v[3 * pa + c] - v[3 * pb + c];
        }
        double *row = W.L + 10 * lane;
        row[0] = dot3_f64(dv[0], dv[0]);
        row[1] = 2.0 * dot3_f64(dv[0], dv[1]);
        row[2] = dot3_f64(dv[1], dv[1]);
        row[3] = 2.0 * dot3_f64(dv[0], dv[2]);
        row[4] = 2.0 * dot3_f64(dv[1], dv[2]);
        row[5] = dot3_f64(dv[2], dv[2]);
        row[6] = 2.0 * dot3_f64(dv[0], dv[3]);
        row[7] = 2.0 * dot3_f64(dv[1], dv[3]);
        row[8] = 2.0 * dot3_f64(dv[2], dv[3]);
        row[9] = dot3_f64(dv[3], dv[3]);
        double d[3];
#pragma unroll
        for (int c = 0; c < 3; c++) d[c] = W.cws[pa][c] - W.cws[pb][c];
        W.rho[lane] = dot3_f64(d, d);
    }
    __syncthreads();
#pragma unroll 1
    for (int br = 0; br < 3; br++) {
        // find_betas_approx_1 / 2 / 3
        const int k = br == 0 ? 4 : br == 1 ? 3 : 5;
        for (int e = lane; e < 6 * k; e += WAVE) {
            const int r = e / k, c = e - r * k;
            W.S[e] = W.L[10 * r + (br == 0 ? (c == 0 ? 0 : c == 1 ? 1 : c == 2 ? 3 : 6) : c)];
        }
        __syncthreads();
        pinv_solve(W, k);
        if (lane == 0) {
            const double *b = W.bx;
            if (br == 0) {
                if (b[0] < 0) {
                    W.betas[0] = sqrt(-b[0]); W.betas[1] = -b[1] / W.betas[0]; W.betas[2] = -b[2] / W.betas[0]; W.betas[3] = -b[3] / W.betas[0];
                } else {
                    W.betas[0] = sqrt(b[0]); W.betas[1] = b[1] / W.betas[0]; W.betas[2] = b[2] / W.betas[0]; W.betas[3] = b[3] / W.betas[0];
                }
            } else {
                if (b[0] < 0) {
                    W.betas[0] = sqrt(-b[0]); W.betas[1] = (b[2] < 0) ? sqrt(-b[2]) : 0.0;
                } else {
                    W.betas[0] = sqrt(b[0]); W.betas[1] = (b[2] > 0) ? sqrt(b[2]) : 0.0;
                }
                if (b[1] < 0) W.betas[0] = -W.betas[0];
                W.betas[2] = br == 2 ? b[3] / W.betas[0] : 0.0;
                W.betas[3] = 0.0;
            }
            gauss_newton(W);
            // compute_ccs, solve_for_sign (the sign of the first correspondence's z; negating the control points negates every pc exactly)
            for (int j = 0; j < 4; j++)
                for (int c = 0; c < 3; c++) {
                    double acc = 0.0;
                    for (int i = 0; i < 4; i++) acc = acc + W.betas[i] * W.ut[12 * (11 - i) + 3 * j + c];
                    W.ccs[j][c] = acc;
                }
            C.load(0, pw, u);
            alphas(W, pw, a);
            if (a[0] * W.ccs[0][2] + a[1] * W.ccs[1][2] + a[2] * W.ccs[2][2] + a[3] * W.ccs[3][2] < 0.0)
                for (int j = 0; j < 4; j++)
                    for (int c = 0; c < 3; c++) W.ccs[j][c] = -W.ccs[j][c];
        }
        __syncthreads();
        // estimate_R_and_t
        if (lane < 3) {
            double acc = 0.0;
            for (int i = 0; i < n; i++) {
                C.load(i, pw, u);
                alphas(W, pw, a);
                acc = acc + (a[0] * W.ccs[0][lane] + a[1] * W.ccs[1][lane] + a[2] * W.ccs[2][lane] + a[3] * W.ccs[3][lane]);
            }
            W.pc0[lane] = acc / dn;
        }
        __syncthreads();
        if (lane < 9) {
            const int j = lane / 3, k2 = lane - 3 * j;
            double acc = 0.0;
            for (int i = 0; i < n; i++) {
                C.load(i, pw, u);
                alphas(W, pw, a);
                const double pc = a[0] * W.ccs[0][j] + a[1] * W.ccs[1][j] + a[2] * W.ccs[2][j] + a[3] * W.ccs[3][j];
                acc = acc + (pc - W.pc0[j]) * ((k2 == 0 ? pw[0] : k2 == 1 ? pw[1] : pw[2]) - W.cws[0][k2]);
            }
            W.S[lane] = acc;
        }
        __syncthreads();
        gram(W, W.S, 3, 3);
        __syncthreads();
        jacobi(W, 3, W.ds, W.uts);
        if (lane < 9) {                                                        // U[i][k] = sum_a ABt[i][a] V[a][k] / sqrt(d_k)
            const int i = lane / 3, k2 = lane - 3 * i;
            double acc = 0.0;
            for (int q = 0; q < 3; q++) acc = acc + W.S[i * 3 + q] * W.uts[k2 * 3 + q];
            W.U[lane] = acc / sqrt(W.ds[k2]);
        }
        __syncthreads();
        if (lane < 9) {                                                        // R = U V^T
            const int i = lane / 3, j = lane - 3 * i;
            double acc = 0.0;
            for (int q = 0; q < 3; q++) acc = acc + W.U[i * 3 + q] * W.uts[q * 3 + j];
            W.R[br][lane] = acc;
        }
        __syncthreads();
        if (lane == 0) {
            double *R = W.R[br], *t = W.t[br];
            const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
            if (det < 0) { R[6] = -R[6]; R[7] = -R[7]; R[8] = -R[8]; }
            t[0] = W.pc0[0] - dot3_f64(R, W.cws[0]); t[1] = W.pc0[1] - dot3_f64(R + 3, W.cws[0]); t[2] = W.pc0[2] - dot3_f64(R + 6, W.cws[0]);
            // reprojection_error
            double sum2 = 0.0;
            for (int i = 0; i < n; i++) {
                C.load(i, pw, u);
                const double Xc = dot3_f64(R, pw) + t[0], Yc = dot3_f64(R + 3, pw) + t[1], inv_Zc = 1.0 / (dot3_f64(R + 6, pw) + t[2]);
                const double ue = uc + fu * Xc * inv_Zc, ve = vc + fv * Yc * inv_Zc;
                sum2 = sum2 + sqrt((u[0] - ue) * (u[0] - ue) + (u[1] - ve) * (u[1] - ve));
            }
            W.err[br] = sum2 / dn;
        }
        __syncthreads();
    }
    if (lane == 0) {
        int N = 0;
        if (W.err[1] < W.err[0]) N = 1;
        if (W.err[2] < W.err[N]) N = 2;
        W.branch = N + 1;
    }
    __syncthreads();
    if (lane < 9) W.Rf[lane] = W.R[W.branch - 1][lane];
    if (lane < 3) W.tf[lane] = W.t[W.branch - 1][lane];
    __syncthreads();
}

// PnPsolver::CheckInliers (:286-312) for the pose W.Rf, W.tf over the pair's N correspondences: the bit mask (words 64-bit words, all
// written) and the count.  Whole wave.
__device__ __forceinline__ int check_inliers(const Work &W, const PnpDev &D, size_t f, int N, unsigned long long *mask) {
    const int lane = threadIdx.x;
    const double fu = D.fx, fv = D.fy, uc = D.cx, vc = D.cy;
    const float *p3d = D.p3d + f * D.cap * 3, *p2d = D.p2d + f * D.cap * 2, *maxErr = D.maxErr + f * D.cap;
    int count = 0;
    for (int w = 0; w < D.words; w++) {
        const int i = w * WAVE + lane;
        bool ok = false;
        if (i < N) {
            const double x = p3d[3 * i], y = p3d[3 * i + 1], z = p3d[3 * i + 2];
            const float Xc = (float)(W.Rf[0] * x + W.Rf[1] * y + W.Rf[2] * z + W.tf[0]);
            const float Yc = (float)(W.Rf[3] * x + W.Rf[4] * y + W.Rf[5] * z + W.tf[1]);
            const float invZc = (float)(1 / (W.Rf[6] * x + W.Rf[7] * y + W.Rf[8] * z + W.tf[2]));
            const double ue = uc + fu * Xc * invZc, ve = vc + fv * Yc * invZc;
            const float distX = (float)(p2d[2 * i] - ue), distY = (float)(p2d[2 * i + 1] - ve);
            const float error2 = distX * distX + distY * distY;
            ok = error2 < maxErr[i];
        }
        const unsigned long long b = __ballot(ok);
        if (lane == 0) mask[w] = b;
        count += __popcll(b);
    }
    return count;
}

__global__ __launch_bounds__(WAVE) void k_pnp_gather(PnpDev D) {
    const size_t f = blockIdx.x;
    const int lane = threadIdx.x;
    int n = D.nKps[f];
    n = n < 0 ? 0 : (n > D.cap ? D.cap : n);
    int run = 0;
    for (int base = 0; base < n; base += WAVE) {
        const int i = base + lane;
        const int m = i < n ? D.match[f * D.cap + i] : -1;
        const bool valid = m >= 0 && m < D.kcap;
        const unsigned long long b = __ballot(valid);
        if (valid) {
            const size_t o = f * D.cap + run + __popcll(b & ((1ull << lane) - 1ull)), g = f * D.cap + i;
            int oct = D.kps[g].octave;
            oct = oct < 0 ? 0 : (oct >= D.nlevels ? D.nlevels - 1 : oct);
            const float *X = D.xyz + (f * D.kcap + m) * 3;
            D.p2d[2 * o] = D.unxy[2 * g]; D.p2d[2 * o + 1] = D.unxy[2 * g + 1];
            D.p3d[3 * o] = X[0]; D.p3d[3 * o + 1] = X[1]; D.p3d[3 * o + 2] = X[2];
            D.maxErr[o] = D.sigma2[oct] * D.th2;
            D.kpIdx[o] = i;
        }
        run += __popcll(b);
    }
    if (lane == 0) {
        const int minInl = D.table[2 * run], maxIts = D.table[2 * run + 1];
        D.N[f] = run;
        D.Kit[f] = run < minInl ? 0 : (maxIts > D.nIter ? maxIts : D.nIter);    // the || of PnPsolver.cc:174
    }
}

__global__ __launch_bounds__(WAVE) void k_pnp_hypothesis(PnpDev D) {
    __shared__ Work W;
    const size_t f = blockIdx.y;
    const int k = blockIdx.x, lane = threadIdx.x;
    const int N = D.N[f];
    if (k >= D.Kit[f]) return;
    if (lane == 0) {                                                           // the sample: swap-with-back removal without the list
        const unsigned h0 = sampler_iteration(D.seed[f], k);
        int pos[4], val[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int r = sampler_draw(h0, j, (unsigned)(N - j));
            int v = r, back = N - 1 - j;
#pragma unroll
            for (int q = 0; q < 4; q++) {                                      // later replacements shadow earlier ones
                if (q < j && pos[q] == r) v = val[q];
                if (q < j && pos[q] == back) back = val[q];
            }
            pos[j] = r; val[j] = back;
            W.idx[j] = v;
        }
    }
    __syncthreads();
    const Corr C{D.p3d + f * D.cap * 3, D.p2d + f * D.cap * 2, W.idx, 4};
    compute_pose(W, C, (double)D.fx, (double)D.fy, (double)D.cx, (double)D.cy);
    const size_t hk = f * D.kmax + k;
    const int count = check_inliers(W, D, f, N, D.mask + hk * D.words);
    if (lane < 9) D.hypRt[hk * 12 + lane] = W.Rf[lane];
    if (lane < 3) D.hypRt[hk * 12 + 9 + lane] = W.tf[lane];
    if (lane == 0) { D.count[hk] = count; D.hypBranch[hk] = W.branch; }
}

__global__ __launch_bounds__(WAVE) void k_pnp_resolve(PnpDev D) {
    __shared__ Work W;
    const size_t f = blockIdx.x;
    const int lane = threadIdx.x;
    const int N = D.N[f], K = D.Kit[f], minInl = D.table[2 * N];
    int32_t *ridx = D.ridx + f * D.cap;
    unsigned long long *rmask = D.rmask + f * D.words;
    int best = 0, bestK = -1, status = 0, nInl = 0;
    for (int k = 0; k < K && status == 0; k++) {
        const int c = D.count[f * D.kmax + k];
        if (c < minInl || c <= best) continue;
        best = c; bestK = k;                                                   // a record: mBestTcw, then Refine() on its inliers
        const unsigned long long *mk = D.mask + (f * D.kmax + k) * D.words;
        int run = 0;
        for (int w = 0; w < D.words; w++) {
            const unsigned long long b = mk[w];
            if (b >> lane & 1ull) ridx[run + __popcll(b & ((1ull << lane) - 1ull))] = w * WAVE + lane;
            run += __popcll(b);
        }
        __syncthreads();
        const Corr C{D.p3d + f * D.cap * 3, D.p2d + f * D.cap * 2, ridx, best};
        compute_pose(W, C, (double)D.fx, (double)D.fy, (double)D.cx, (double)D.cy);
        const int rc = check_inliers(W, D, f, N, rmask);
        if (rc > minInl) { status = 1; nInl = rc; }
        __syncthreads();
    }
    const unsigned long long *fm = rmask;
    if (status == 0 && bestK >= 0) {                                           // bNoMore: the best unrefined pose
        status = 2; nInl = best; fm = D.mask + (f * D.kmax + bestK) * D.words;
        if (lane < 12) (lane < 9 ? W.Rf[lane] : W.tf[lane - 9]) = D.hypRt[(f * D.kmax + bestK) * 12 + lane];
    }
    __syncthreads();
    for (int i = lane; i < D.cap; i += WAVE) { D.inlier[f * D.cap + i] = 0; D.ptRef[f * D.cap + i] = -1; }
    __syncthreads();
    if (status != 0)
        for (int i = lane; i < N; i += WAVE)
            if (fm[i >> 6] >> (i & 63) & 1ull) {
                const size_t g = f * D.cap + D.kpIdx[f * D.cap + i];
                D.inlier[g] = 1; D.ptRef[g] = D.match[g];
            }
    if (lane < 12) {
        const int r = lane >> 2, c = lane & 3;
        D.Tcw[f * 12 + lane] = status == 0 ? (r == c ? 1.0f : 0.0f) : (c < 3 ? (float)W.Rf[3 * r + c] : (float)W.tf[r]);
    }
    if (lane == 0) { D.nInl[f] = nInl; D.status[f] = status; }
}

// SetRansacParameters (PnPsolver.cc:128-147) for N correspondences, with the host's libm as the reference evaluates it.
void ransac_entry(const msl_pnp_params &p, int N, int32_t *out) {
    float eps = p.epsilon;
    int nMin = (int)((float)N * eps);
    if (nMin < p.min_inliers) nMin = p.min_inliers;
    if (nMin < p.min_set) nMin = p.min_set;
    out[0] = nMin; out[1] = 1;
    if (N < nMin) return;                                                      // no pose: the count is not used
    if (eps < (float)nMin / (float)N) eps = (float)nMin / (float)N;
    double it = 1.0;
    if (nMin != N) it = std::ceil(std::log(1 - p.probability) / std::log(1 - std::pow((double)eps, 3.0)));
    if (it != it) it = 1.0;                                                    // pin: an undefined count is 1
    const int n = it >= (double)p.max_iterations ? p.max_iterations : (it < 1.0 ? 1 : (int)it);
    out[1] = n < 1 ? 1 : n;
}

size_t carve(size_t &off, size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; }

constexpr const char *WHO = "msl_pnp_ransac";

int check_pnp(int n_pairs, int cap, int kcap, const msl_pnp_params *params, const msl_keypoint *kps, const float *un_xy, const int32_t *match,
              const int32_t *n_kps, const float *xyz, const uint32_t *seed, msl_mem, float *Tcw_out, uint8_t *inlier, int32_t *pt_ref_out,
              int32_t *n_inliers, int32_t *status, msl_mem) {
    if (!none_null(WHO, {MSL_NAMED(params), MSL_NAMED(kps), MSL_NAMED(un_xy), MSL_NAMED(match), MSL_NAMED(n_kps), MSL_NAMED(xyz), MSL_NAMED(seed),
                         MSL_NAMED(Tcw_out), MSL_NAMED(inlier), MSL_NAMED(pt_ref_out), MSL_NAMED(n_inliers), MSL_NAMED(status)})) return MSL_ERR_INVALID;
    if (!at_least_one(WHO, "n_pairs", n_pairs)) return MSL_ERR_INVALID;
    if (cap < 1 || cap > MAX_CAP) { set_error("%s: cap %d outside 1 .. %d", WHO, cap, MAX_CAP); return MSL_ERR_INVALID; }
    if (kcap < 1 || kcap > MAX_KCAP) { set_error("%s: kcap %d outside 1 .. %d", WHO, kcap, MAX_KCAP); return MSL_ERR_INVALID; }
    if (params->min_set != 4) { set_error("%s: min_set %d (only 4, the reference's one use, is built)", WHO, params->min_set); return MSL_ERR_INVALID; }
    if (params->nlevels < 1 || params->nlevels > MSL_MATCH_MAX_LEVELS) {
        set_error("%s: nlevels %d outside 1 .. %d", WHO, params->nlevels, MSL_MATCH_MAX_LEVELS);
        return MSL_ERR_INVALID;
    }
    if (params->max_iterations < 1 || params->max_iterations > MAX_ITS) {
        set_error("%s: max_iterations %d outside 1 .. %d", WHO, params->max_iterations, MAX_ITS);
        return MSL_ERR_INVALID;
    }
    if (params->n_iterations < 0 || params->n_iterations > MAX_ITS) {
        set_error("%s: n_iterations %d outside 0 .. %d", WHO, params->n_iterations, MAX_ITS);
        return MSL_ERR_INVALID;
    }
    return MSL_OK;
}

int launch_pnp(msl_match *h, int n_pairs, int cap, int kcap, const msl_pnp_params *prm, const msl_keypoint *kps, const float *un_xy,
               const int32_t *match, const int32_t *n_kps, const float *xyz, const uint32_t *seed, msl_mem mem, float *Tcw_out, uint8_t *inlier,
               int32_t *pt_ref_out, int32_t *n_inliers, int32_t *status, msl_mem out_mem) {
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    hipStream_t st = h->stream;
    const size_t P = (size_t)n_pairs, n = P * cap;
    PnpDev D{};
    D.cap = cap; D.kcap = kcap; D.kmax = prm->max_iterations > prm->n_iterations ? prm->max_iterations : prm->n_iterations;
    D.words = (cap + WAVE - 1) / WAVE; D.nIter = prm->n_iterations; D.nlevels = prm->nlevels;
    D.fx = prm->fx; D.fy = prm->fy; D.cx = prm->cx; D.cy = prm->cy; D.th2 = prm->th2;
    for (int i = 0; i < MSL_MATCH_MAX_LEVELS; i++) D.sigma2[i] = prm->level_sigma2[i];
    // the table N -> (minInliers, maxIts): rebuilt and uploaded when the RANSAC parameters or cap change
    const PnpKey key{prm->probability, prm->min_inliers, prm->max_iterations, prm->min_set, prm->epsilon, cap, 0};
    if (!h->pnpTableValid || std::memcmp(&key, &h->pnpKey, sizeof key) != 0) {
        std::vector<int32_t> table(2 * ((size_t)cap + 1));
        for (int N = 0; N <= cap; N++) ransac_entry(*prm, N, &table[2 * (size_t)N]);
        h->pnpTableValid = false;
        MSL_HIP_TRY(h->pnpTable.grow(table.size() * sizeof(int32_t), st));
        MSL_HIP_TRY(hipMemcpyAsync(h->pnpTable.p, table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
        MSL_HIP_TRY(hipStreamSynchronize(st));                                 // `table` is released on return
        h->pnpKey = key; h->pnpTableValid = true;
    }
    D.table = (const int32_t *)h->pnpTable.p;
    const size_t HK = P * D.kmax;
    size_t off = 0;
    const size_t oP2d = carve(off, n * 2 * sizeof(float)), oP3d = carve(off, n * 3 * sizeof(float)), oErr = carve(off, n * sizeof(float)),
                 oIdx = carve(off, n * sizeof(int32_t)), oN = carve(off, P * sizeof(int32_t)), oK = carve(off, P * sizeof(int32_t)),
                 oMask = carve(off, HK * D.words * sizeof(unsigned long long)), oCnt = carve(off, HK * sizeof(int32_t)),
                 oRt = carve(off, HK * 12 * sizeof(double)), oBr = carve(off, HK * sizeof(int32_t)), oRidx = carve(off, n * sizeof(int32_t)),
                 oRmask = carve(off, P * D.words * sizeof(unsigned long long));
    MSL_HIP_TRY(h->pnp.grow(off, st));
    char *base = (char *)h->pnp.p;
    D.p2d = (float *)(base + oP2d); D.p3d = (float *)(base + oP3d); D.maxErr = (float *)(base + oErr); D.kpIdx = (int32_t *)(base + oIdx);
    D.N = (int32_t *)(base + oN); D.Kit = (int32_t *)(base + oK); D.mask = (unsigned long long *)(base + oMask); D.count = (int32_t *)(base + oCnt);
    D.hypRt = (double *)(base + oRt); D.hypBranch = (int32_t *)(base + oBr); D.ridx = (int32_t *)(base + oRidx);
    D.rmask = (unsigned long long *)(base + oRmask);
    h->pnpPairs = n_pairs; h->pnpKmax = D.kmax; h->pnpOffK = oK; h->pnpOffCnt = oCnt; h->pnpOffRt = oRt; h->pnpOffBr = oBr;
    Stage S(h, mem, out_mem);
    D.kps = S.in(kps, n); D.unxy = S.in(un_xy, 2 * n); D.match = S.in(match, n); D.nKps = S.in(n_kps, P); D.xyz = S.in(xyz, 3 * P * kcap);
    D.seed = S.in(seed, P);
    D.Tcw = S.out(Tcw_out, 12 * P); D.inlier = S.out(inlier, n); D.ptRef = S.out(pt_ref_out, n); D.nInl = S.out(n_inliers, P);
    D.status = S.out(status, P);
    MSL_HIP_TRY(S.error());
    hipLaunchKernelGGL(k_pnp_gather, dim3((unsigned)n_pairs), dim3(WAVE), 0, st, D);
    MSL_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_pnp_hypothesis, dim3((unsigned)D.kmax, (unsigned)n_pairs), dim3(WAVE), 0, st, D);
    MSL_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_pnp_resolve, dim3((unsigned)n_pairs), dim3(WAVE), 0, st, D);
    MSL_HIP_TRY(hipGetLastError());
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}

}  // namespace

extern "C" {

int msl_pnp_ransac(msl_match *h, int n_pairs, int cap, int kcap, const msl_pnp_params *params, const msl_keypoint *kps, const float *un_xy,
                   const int32_t *match, const int32_t *n_kps, const float *xyz, const uint32_t *seed, msl_mem mem, float *Tcw_out, uint8_t *inlier,
                   int32_t *pt_ref_out, int32_t *n_inliers, int32_t *status, msl_mem out_mem) noexcept {
    try {
    return handle_form(WHO, check_pnp, launch_pnp, h, n_pairs, cap, kcap, params, kps, un_xy, match, n_kps, xyz, seed, mem, Tcw_out, inlier, pt_ref_out,
                       n_inliers, status, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_pnp_ransac_batch(int device, int n_pairs, int cap, int kcap, const msl_pnp_params *params, const msl_keypoint *kps, const float *un_xy,
                         const int32_t *match, const int32_t *n_kps, const float *xyz, const uint32_t *seed, msl_mem mem, float *Tcw_out,
                         uint8_t *inlier, int32_t *pt_ref_out, int32_t *n_inliers, int32_t *status, msl_mem out_mem) noexcept {
    try {
    return batch_form(check_pnp, launch_pnp, device, mem == MSL_MEM_DEVICE || out_mem == MSL_MEM_DEVICE, n_pairs, cap, kcap, params, kps, un_xy, match, n_kps,
                      xyz, seed, mem, Tcw_out, inlier, pt_ref_out, n_inliers, status, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_pnp_debug_hypotheses(msl_match *h, int pair, int kcap_out, double *R, double *t, int32_t *branch, int32_t *count, int32_t *n_out) noexcept {
    try {
    if (!h || !R || !t || !branch || !count || !n_out || kcap_out < 0 || pair < 0 || pair >= h->pnpPairs || !h->pnp.p) {
        set_error("msl_pnp_debug_hypotheses: invalid argument (pair outside the last msl_pnp_ransac call?)");
        return MSL_ERR_INVALID;
    }
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    MSL_HIP_TRY(hipStreamSynchronize(h->stream));
    const char *base = (const char *)h->pnp.p;
    int32_t K = 0;
    MSL_HIP_TRY(hipMemcpy(&K, base + h->pnpOffK + sizeof(int32_t) * (size_t)pair, sizeof K, hipMemcpyDeviceToHost));
    *n_out = K;
    const size_t nk = (size_t)(K < kcap_out ? K : kcap_out), hk = (size_t)pair * h->pnpKmax;
    if (!nk) return MSL_OK;
    std::vector<double> rt(12 * nk);
    MSL_HIP_TRY(hipMemcpy(rt.data(), base + h->pnpOffRt + hk * 12 * sizeof(double), rt.size() * sizeof(double), hipMemcpyDeviceToHost));
    MSL_HIP_TRY(hipMemcpy(branch, base + h->pnpOffBr + hk * sizeof(int32_t), nk * sizeof(int32_t), hipMemcpyDeviceToHost));
    MSL_HIP_TRY(hipMemcpy(count, base + h->pnpOffCnt + hk * sizeof(int32_t), nk * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < nk; k++) {
        for (int i = 0; i < 9; i++) R[9 * k + i] = rt[12 * k + i];
        for (int i = 0; i < 3; i++) t[3 * k + i] = rt[12 * k + 9 + i];
    }
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}

}  // extern "C"

// msl_line3d.hip -- batched 3-D line reconstruction for gfx950: Frame::GetLineDepth (reference src/Frame.cc:179-186), Frame::Obtain3DLine
// (:528-603) with all of src/3DLineExtractor.cpp, and the line half of its three call sites (src/Tracking.cc:575-592, :1107-1143,
// :1569-1618): msl_lines_3d[_batch].
//
// Kernels (one wave per workgroup):
//   k_line3d         one wave per keyline: the end-point depths, the <= 128 samples along the keyline (two per lane: position and DU in
//                    registers, positions also in LDS), the RANSAC of extract3dline_mahdist with inlier sets as two ballot masks, verify3dLine,
//                    the refit loop, the end points, the acceptance test and the world transform
//   k_line3d_select  one wave per frame: the call site's walk (index order or ascending (min end depth, index), ranked by counting) with its
//                    `nLines > max_new_lines` stop -> line_new, n_new
//
// Pins where the reference is undefined or not restated (tests/line3d_model.py is the
// sequential model and the kernel runs every sum in the order that model states):
//   * cv::SVD: both uses are the cyclic Jacobi eigen-solver of msl_jacobi.h on a symmetric 3x3 matrix (jacobi_sweep<3>, in registers: the
//     round-robin steps are the pairs (1,2), (0,2), (0,1); 16 sweeps; eigenpairs by descending eigenvalue, no sign normalisation).  For a sample
//     the matrix is cov0 (its upper triangle mirrored), DU = diag(1 / sqrt(w)) U^T; for the refit it is P^T P of the centred inliers with
//     left-to-right sums in ascending sample order, the direction its top eigenvector.  The sign of d only swaps A and B.
//   * rand() % left: draw j of iteration k = msl_match_math.h's sampler_draw (the sampler of msl_pnp_ransac); one seed per keyline
//   * the "NULL" Vector6d: line_ok says whether a line was returned; line_xyz of a failed keyline is six zeros
//   * numSmp == 0 (a division by zero) and fewer than min_points samples: no line
//   * GetLineDepth outside the image: -1.0f
//   * non-finite values propagate by IEEE rules; a NaN distance is not an inlier; a NaN sample position is dropped by the bounds test
#include "msl_jacobi.h"
#include "msl_match_handle.h"
#include "msl_match_math.h"

#include <climits>
#include <cmath>
#include <vector>

namespace {

using namespace msl;

constexpr int MAX_SAMPLES = 127, MAX_ITERS = 64, NS = 128;
constexpr double L3_EPS = 1e-10;             // 3DLineExtractor.h's EPS

// What msl_lines_3d_debug reads back per keyline.
struct LineDbg {
    int32_t nKept, nIter, refits, end[2], pad[3];
    int32_t it[MAX_ITERS][4];                // the two drawn sample indices, the inlier count (-1: |B - A| < EPS), record
    double m[3], d[3];
};

struct Line3dDev {
    int lcap, order, width, height;
    float fx, cx, cy, invfx, invfy;
    int maxSamples, minPoints, maxIter, maxNew;
    double distTh, minSupport, minLength;
    const float *ends; const int32_t *nLines; const uint8_t *depth; size_t rowStride, frameStride;
    const uint8_t *flags; const float *Tcw; const uint32_t *seed;
    float *lineDepth; double *xyz; uint8_t *ok, *isNew; int32_t *nSupport, *nNew;
    LineDbg *dbg;
};

struct V3 { double x, y, z; };
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator*(V3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ double norm(V3 a) { return sqrt(a.x * a.x + a.y * a.y + a.z * a.z); }

struct L3Work {
    double pos[NS][3];
    int idx[NS];                             // extract3dline_mahdist's `indexes`, carried across the iterations
    double mean[3], G[9];
    int ia, ib;
};

__device__ __forceinline__ V3 sample(const L3Work &W, int k) { return {W.pos[k][0], W.pos[k][1], W.pos[k][2]}; }

// Eigenpairs of the symmetric 3x3 A, in registers: d[3] descending (the lower index first on ties), ut[3][3] with the eigenvectors as rows.
// msl_jacobi.h's sweeps from V = identity, then the ranking by counting.
__device__ __forceinline__ void jacobi3(double (&A)[9], double (&d)[3], double (&ut)[9]) {
    double V[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
#pragma unroll 1
    for (int sw = 0; sw < JACOBI_SWEEPS; sw++) jacobi_sweep<3>(A, V);
    const double d0 = A[0], d1 = A[4], d2 = A[8];
    const int r0 = (d1 > d0 ? 1 : 0) + (d2 > d0 ? 1 : 0);
    const int r1 = ((d0 > d1 || d0 == d1) ? 1 : 0) + (d2 > d1 ? 1 : 0);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        d[k] = r0 == k ? d0 : (r1 == k ? d1 : d2);                                // the third takes the rank that is left
#pragma unroll
        for (int a = 0; a < 3; a++) ut[k * 3 + a] = r0 == k ? V[a * 3] : (r1 == k ? V[a * 3 + 1] : V[a * 3 + 2]);
    }
}

// compPt3dCov: DU = diag(1 / sqrt(w)) U^T of cov0 = J0 diag(1, 1, sigma(z)^2) J0^T (f = fx for both rows, as in the file).
__device__ __forceinline__ void sample_du(V3 p, double f, double (&DU)[9]) {
    const double s = 0.00273 * p.z * p.z + 0.00074 * p.z + -0.00058;       // depthStdDev
    const double s2 = s * s;
    const double a = p.z / f, bx = p.x / p.z, by = p.y / p.z;
    const double mx = bx * s2, my = by * s2;                                  // (J0 cov_g)[0][2], [1][2]
    double A[9], d[3], ut[9];
    A[0] = a * a + mx * bx; A[1] = mx * by; A[2] = mx;
    A[4] = a * a + my * by; A[5] = my;
    A[8] = s2;
    A[3] = A[1]; A[6] = A[2]; A[7] = A[5];
    jacobi3(A, d, ut);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double w = 1.0 / sqrt(d[i]);
#pragma unroll
        for (int j = 0; j < 3; j++) DU[i * 3 + j] = w * ut[i * 3 + j];
    }
}

// mah_dist3d_pt_line in the file's operation order.
__device__ __forceinline__ double mah_dist(V3 p, const double (&c)[9], V3 q1, V3 q2) {
    const double xa = q1.x, ya = q1.y, za = q1.z, xb = q2.x, yb = q2.y, zb = q2.z;
    const double c1 = c[0], c2 = c[1], c3 = c[2], c4 = c[3], c5 = c[4], c6 = c[5], c7 = c[6], c8 = c[7], c9 = c[8];
    const double x1 = p.x, x2 = p.y, x3 = p.z;
    const double term1 = ((c1 * (x1 - xa) + c2 * (x2 - ya) + c3 * (x3 - za)) * (c4 * (x1 - xb) + c5 * (x2 - yb) + c6 * (x3 - zb))
                          - (c4 * (x1 - xa) + c5 * (x2 - ya) + c6 * (x3 - za)) * (c1 * (x1 - xb) + c2 * (x2 - yb) + c3 * (x3 - zb))),
                 term2 = ((c1 * (x1 - xa) + c2 * (x2 - ya) + c3 * (x3 - za)) * (c7 * (x1 - xb) + c8 * (x2 - yb) + c9 * (x3 - zb))
                          - (c7 * (x1 - xa) + c8 * (x2 - ya) + c9 * (x3 - za)) * (c1 * (x1 - xb) + c2 * (x2 - yb) + c3 * (x3 - zb))),
                 term3 = ((c4 * (x1 - xa) + c5 * (x2 - ya) + c6 * (x3 - za)) * (c7 * (x1 - xb) + c8 * (x2 - yb) + c9 * (x3 - zb))
                          - (c7 * (x1 - xa) + c8 * (x2 - ya) + c9 * (x3 - za)) * (c4 * (x1 - xb) + c5 * (x2 - yb) + c6 * (x3 - zb))),
                 term4 = (c1 * (x1 - xa) - c1 * (x1 - xb) + c2 * (x2 - ya) - c2 * (x2 - yb) + c3 * (x3 - za) - c3 * (x3 - zb)),
                 term5 = (c4 * (x1 - xa) - c4 * (x1 - xb) + c5 * (x2 - ya) - c5 * (x2 - yb) + c6 * (x3 - za) - c6 * (x3 - zb)),
                 term6 = (c7 * (x1 - xa) - c7 * (x1 - xb) + c8 * (x2 - ya) - c8 * (x2 - yb) + c9 * (x3 - za) - c9 * (x3 - zb));
    return sqrt((term1 * term1 + term2 * term2 + term3 * term3) / (term4 * term4 + term5 * term5 + term6 * term6));
}

// projectPt3d2Ln3d
__device__ __forceinline__ V3 project(V3 P, V3 mid, V3 drct) {
    const V3 A = mid, B = mid + drct, AB = B - A, AP = P - A;
    return A + AB * (dot(AB, AP) / dot(AB, AB));
}

// The lane's two samples: k0 = lane, k1 = lane + 64; in0 / in1 say which of them belong to the set that is scanned.
struct Pair { V3 p0, p1; int k0, k1; };

// The `minv = 100; if (v < minv)` scan of the reference over a set in ascending sample order: the first sample that attains the smallest v
// among those with v < 100, or `first` (the set's first sample, the scan's idx = 0) when no v is below 100.  Whole wave.
__device__ __forceinline__ int scan_min(double v0, bool in0, int k0, double v1, bool in1, int k1, int first) {
    double v = 100.0; int k = INT_MAX;
    if (in0 && v0 < v) { v = v0; k = k0; }
    if (in1 && v1 < v) { v = v1; k = k1; }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(v, off); const int ok = __shfl_xor(k, off);
        if (ov < v || (ov == v && ok < k)) { v = ov; k = ok; }
    }
    return k == INT_MAX ? first : k;
}

// Both extremes of the set (m0, m1) along `dir` from `origin`; `maxv = -100; if (v > maxv)` is the same scan on -v.
__device__ __forceinline__ void extremes(const Pair &S, unsigned long long m0, unsigned long long m1, V3 origin, V3 dir, int &i1, int &i2) {
    const int lane = threadIdx.x;
    const bool in0 = m0 >> lane & 1ull, in1 = m1 >> lane & 1ull;
    const int first = m0 ? __ffsll((long long)m0) - 1 : 64 + __ffsll((long long)m1) - 1;
    const double v0 = dot(S.p0 - origin, dir), v1 = dot(S.p1 - origin, dir);
    i1 = scan_min(v0, in0, S.k0, v1, in1, S.k1, first);
    i2 = scan_min(-v0, in0, S.k0, -v1, in1, S.k1, first);
}

// verify3dLine over the set (m0, m1).  Whole wave.
__device__ __forceinline__ bool verify_line(const L3Work &W, const Pair &S, unsigned long long m0, unsigned long long m1, V3 A, V3 B) {
    const int lane = threadIdx.x;
    const V3 AB = B - A;
    int i1, i2;
    extremes(S, m0, m1, A, AB, i1, i2);
    const V3 mid = (A + B) * 0.5;
    const V3 C = project(sample(W, i1), mid, AB), Dp = project(sample(W, i2), mid, AB);
    const V3 DC = Dp - C;
    const double cd = norm(DC);
    if (cd < L3_EPS) return false;
    unsigned cells = 0;
    if (m0 >> lane & 1ull) { const double lam = fabs(dot(S.p0 - C, DC) / cd / cd); cells |= 1u << (lam >= 1 ? 9 : ((int)floor(lam * 10) & 15)); }
    if (m1 >> lane & 1ull) { const double lam = fabs(dot(S.p1 - C, DC) / cd / cd); cells |= 1u << (lam >= 1 ? 9 : ((int)floor(lam * 10) & 15)); }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) cells |= (unsigned)__shfl_xor((int)cells, off);
    const double sum = (double)__popc(cells & 0x3FFu);
    return sum / 10 > 0.7;
}

// The samples of (m0, m1) within dist_thresh of the line (q1, q2): the new masks, and their count.  Whole wave.
__device__ __forceinline__ int inliers(const Pair &S, const double (&DU0)[9], const double (&DU1)[9], int n, V3 q1, V3 q2, double th,
                                       unsigned long long &m0, unsigned long long &m1) {
    const bool a = S.k0 < n && mah_dist(S.p0, DU0, q1, q2) < th, b = S.k1 < n && mah_dist(S.p1, DU1, q1, q2) < th;
    m0 = __ballot(a); m1 = __ballot(b);
    return __popcll(m0) + __popcll(m1);
}

__device__ __forceinline__ float depth_at(const Line3dDev &D, size_t f, int row, int col) {
    return *(const float *)(D.depth + f * D.frameStride + (size_t)row * D.rowStride + (size_t)col * sizeof(float));
}

// imDepth.at<float>(y, x) with the truncating conversion; -1.0f outside the image (pin)
__device__ __forceinline__ float end_depth(const Line3dDev &D, size_t f, float x, float y) {
    if (!(fabsf(x) < 2147483648.0f) || !(fabsf(y) < 2147483648.0f)) return -1.0f;
    const int c = (int)x, r = (int)y;
    if (r < 0 || c < 0 || r >= D.height || c >= D.width) return -1.0f;
    return depth_at(D, f, r, c);
}

__global__ __launch_bounds__(WAVE) void k_line3d(Line3dDev D) {
    __shared__ L3Work W;
    const size_t f = blockIdx.y;
    const int j = blockIdx.x, lane = threadIdx.x;
    const size_t g = f * D.lcap + j;
    LineDbg &dbg = D.dbg[g];
    int nl = D.nLines[f];
    nl = nl < 0 ? 0 : (nl > D.lcap ? D.lcap : nl);
    const float *e = D.ends + g * 4;
    float z0 = -1.0f, z1 = -1.0f;
    bool cand = false;
    if (j < nl) {
        z0 = end_depth(D, f, e[0], e[1]); z1 = end_depth(D, f, e[2], e[3]);
        const int fl = D.flags ? D.flags[g] : 0;
        cand = z0 > 0 && z1 > 0 && (D.order == MSL_LINE3D_ALL || (fl & 3) != 3);
    }
    // what a keyline without a line leaves behind; lane 0 writes every output once, at the end
    int ok = 0, support = 0, nIter = 0, refits = 0, end1 = 0, end2 = 0;
    V3 m{0.0, 0.0, 0.0}, d{0.0, 0.0, 0.0};
    float Aw[3] = {0.0f, 0.0f, 0.0f}, Bw[3] = {0.0f, 0.0f, 0.0f};
    const float sx = e[0], sy = e[1], ex = e[2], ey = e[3];
    const float dx = sx - ex, dy = sy - ey;
    const double len = sqrt((double)dx * (double)dx + (double)dy * (double)dy);
    int num = 0;                                                                  // numSmp
    if (cand && len <= 1.7e308) num = len >= (double)D.maxSamples ? D.maxSamples : (int)len;
    // ---- the samples: j = lane and lane + 64 of 0 .. numSmp ----
    V3 q[2]; bool keep[2];
#pragma unroll
    for (int s = 0; s < 2; s++) {
        const int jj = lane + WAVE * s;
        keep[s] = false; q[s] = {0.0, 0.0, 0.0};
        if (num > 0 && jj <= num) {
            const double t = (double)jj / (double)num, a = 1 - t;
            const float px = (float)((double)sx * a) + (float)((double)ex * t), py = (float)((double)sy * a) + (float)((double)ey * t);
            const double x = px, y = py;
            if (x >= 0 && y >= 0 && x < (double)D.width && y < (double)D.height) {
                int col, row;
                if (floor(x) == x && floor(y) == y) { col = max((int)(x - 1), 0); row = max((int)(y - 1), 0); }
                else { col = (int)x; row = (int)y; }
                const float d = depth_at(D, f, row, col);
                if (!((double)d <= 0.01)) {
                    const double z = d;
                    keep[s] = true;
                    q[s] = {(double)((float)col - D.cx) * z * (double)D.invfx, (double)((float)row - D.cy) * z * (double)D.invfy, z};
                }
            }
        }
    }
    const unsigned long long b0 = __ballot(keep[0]), b1 = __ballot(keep[1]), below = (1ull << lane) - 1ull;
    const int n = __popcll(b0) + __popcll(b1);
    if (keep[0]) { const int k = __popcll(b0 & below); W.pos[k][0] = q[0].x; W.pos[k][1] = q[0].y; W.pos[k][2] = q[0].z; }
    if (keep[1]) { const int k = __popcll(b0) + __popcll(b1 & below); W.pos[k][0] = q[1].x; W.pos[k][1] = q[1].y; W.pos[k][2] = q[1].z; }
    for (int i = lane; i < NS; i += WAVE) W.idx[i] = i;
    __syncthreads();
    if (n >= D.minPoints) {                                                        // uniform: the whole wave takes the same side
        Pair S;
        S.k0 = lane; S.k1 = lane + WAVE;
        S.p0 = S.k0 < n ? sample(W, S.k0) : V3{0.0, 0.0, 1.0};
        S.p1 = S.k1 < n ? sample(W, S.k1) : V3{0.0, 0.0, 1.0};
        double DU0[9], DU1[9];
        sample_du(S.p0, (double)D.fx, DU0);
        sample_du(S.p1, (double)D.fx, DU1);
        // ---- extract3dline_mahdist ----
        const double th = D.distTh;
        const int half = (int)((double)((size_t)n * (size_t)(n - 1)) * 0.5);
        const int maxIt = D.maxIter < half ? D.maxIter : half;
        const unsigned seed = D.seed[g];
        int best = 0, bestA = 0, bestB = 0;
        unsigned long long bm0 = 0, bm1 = 0;
        for (int it = 0; it < maxIt; it++) {
            nIter = it + 1;
            if (lane == 0) {                                                       // random_unique(indexes, 2)
                const unsigned h0 = fmix32(seed ^ (unsigned)it * 0x9E3779B1u);    // = sampler_iteration(seed, it)
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    const int r = sampler_draw(h0, u, (unsigned)(n - u));
                    const int t = W.idx[u]; W.idx[u] = W.idx[u + r]; W.idx[u + r] = t;
                }
                W.ia = W.idx[0]; W.ib = W.idx[1];
            }
            __syncthreads();
            const int ia = W.ia, ib = W.ib;
            __syncthreads();
            const V3 A = sample(W, ia), B = sample(W, ib);
            if (norm(B - A) < L3_EPS) {
                if (lane == 0) { dbg.it[it][0] = ia; dbg.it[it][1] = ib; dbg.it[it][2] = -1; dbg.it[it][3] = 0; }
                continue;
            }
            unsigned long long m0, m1;
            const int cnt = inliers(S, DU0, DU1, n, A, B, th, m0, m1);
            int record = 0;
            if (cnt > best && verify_line(W, S, m0, m1, A, B)) { best = cnt; bm0 = m0; bm1 = m1; bestA = ia; bestB = ib; record = 1; }
            if (lane == 0) { dbg.it[it][0] = ia; dbg.it[it][1] = ib; dbg.it[it][2] = cnt; dbg.it[it][3] = record; }
            if ((double)best > (double)n * 0.6) break;
        }
        V3 A{0.0, 0.0, 0.0}, B{0.0, 0.0, 0.0};
        if (best >= 2) {
            const V3 pa = sample(W, bestA), pb = sample(W, bestB);
            m = (pa + pb) * 0.5; d = pb - pa;
            while (true) {
                refits++;
                __syncthreads();
                // computeLine3d_svd: the mean, then P^T P, one entry per lane, over the set in ascending order
                if (lane < 3) {
                    double acc = 0.0;
                    for (unsigned long long b = bm0; b; b &= b - 1) acc = acc + W.pos[__ffsll((long long)b) - 1][lane];
                    for (unsigned long long b = bm1; b; b &= b - 1) acc = acc + W.pos[63 + __ffsll((long long)b)][lane];
                    W.mean[lane] = acc * (1.0 / best);
                }
                __syncthreads();
                if (lane < 9) {
                    const int a = lane / 3, c = lane - 3 * a;
                    const double ma = W.mean[a], mc = W.mean[c];
                    double acc = 0.0;
                    for (unsigned long long b = bm0; b; b &= b - 1) { const int k = __ffsll((long long)b) - 1; acc = acc + (W.pos[k][a] - ma) * (W.pos[k][c] - mc); }
                    for (unsigned long long b = bm1; b; b &= b - 1) { const int k = 63 + __ffsll((long long)b); acc = acc + (W.pos[k][a] - ma) * (W.pos[k][c] - mc); }
                    W.G[lane] = acc;
                }
                __syncthreads();
                double G[9], ev[3], ut[9];
#pragma unroll
                for (int i = 0; i < 9; i++) G[i] = W.G[i];
                jacobi3(G, ev, ut);
                const V3 tm{W.mean[0], W.mean[1], W.mean[2]}, td{ut[0], ut[1], ut[2]};
                unsigned long long t0, t1;
                const int cnt = inliers(S, DU0, DU1, n, tm, tm + td, th, t0, t1);
                if (cnt > best) { best = cnt; bm0 = t0; bm1 = t1; m = tm; d = td; }
                else break;
            }
            extremes(S, bm0, bm1, m, d, end1, end2);
            A = sample(W, end1); B = sample(W, end2);
        }
        support = best;
        // ---- Obtain3DLine's acceptance and the world transform ----
        if ((double)best / len > D.minSupport && norm(A - B) > D.minLength) {
            ok = 1;
            const float *Tc = D.Tcw + f * 12;
            float Ow[3];
            camera_centre(Tc, Ow);                                                 // mOw = -mRcw.t() * mtcw
            const float Ac[3] = {(float)A.x, (float)A.y, (float)A.z}, Bc[3] = {(float)B.x, (float)B.y, (float)B.z};
            gemm3(Tc, true, 1.0, Ac, Ow, Aw);                                      // mRwc * Ac + mOw
            gemm3(Tc, true, 1.0, Bc, Ow, Bw);
        }
    }
    if (lane == 0) {
        D.lineDepth[2 * g] = z0; D.lineDepth[2 * g + 1] = z1;
        for (int i = 0; i < 3; i++) { D.xyz[6 * g + i] = (double)Aw[i]; D.xyz[6 * g + 3 + i] = (double)Bw[i]; }
        D.ok[g] = (uint8_t)ok; D.nSupport[g] = support;
        dbg.nKept = n; dbg.nIter = nIter; dbg.refits = refits; dbg.end[0] = end1; dbg.end[1] = end2; dbg.pad[0] = dbg.pad[1] = dbg.pad[2] = 0;
        dbg.m[0] = m.x; dbg.m[1] = m.y; dbg.m[2] = m.z; dbg.d[0] = d.x; dbg.d[1] = d.y; dbg.d[2] = d.z;
    }
}

// The walk of the call site over one frame's keylines (the per-keyline results are complete).
__global__ __launch_bounds__(WAVE) void k_line3d_select(Line3dDev D) {
    __shared__ float key[MAX_KLCAP];
    __shared__ int ord[MAX_KLCAP];
    __shared__ uint8_t member[MAX_KLCAP], isNew[MAX_KLCAP];
    const size_t f = blockIdx.x;
    const int lane = threadIdx.x;
    int nl = D.nLines[f];
    nl = nl < 0 ? 0 : (nl > D.lcap ? D.lcap : nl);
    for (int i = lane; i < MAX_KLCAP; i += WAVE) {
        bool both = false; float k = 0.0f;
        if (i < nl) {
            const float z0 = D.lineDepth[2 * (f * D.lcap + i)], z1 = D.lineDepth[2 * (f * D.lcap + i) + 1];
            both = z0 > 0 && z1 > 0;
            if (both && D.order == MSL_LINE3D_DEPTH_ORDER) k = z1 < z0 ? z1 : z0;  // std::min
        }
        member[i] = both; key[i] = k; isNew[i] = 0;
    }
    __syncthreads();
    int total = 0;
    if (D.order == MSL_LINE3D_ALL) {
        for (int i = lane; i < nl; i += WAVE) { const bool v = member[i] && D.ok[f * D.lcap + i]; isNew[i] = v; total += v; }
    } else {
        // the position of every member in the walk: the members that sort before it (sort of pair<float, int>), counted
        int M = 0;
        for (int i = lane; i < MAX_KLCAP; i += WAVE) {
            int rank = 0;
            const float ki = key[i];
            for (int o = 0; o < nl; o++) rank += member[o] && (key[o] < ki || (key[o] == ki && o < i)) ? 1 : 0;
            if (member[i]) ord[rank] = i;
            M += __popcll(__ballot(member[i] != 0));
        }
        __syncthreads();
        int run = 0;                                                               // nLines before this chunk of the walk
        for (int base = 0; base < M; base += WAVE) {
            const int p = base + lane;
            bool counts = false, fresh = false;
            int i = 0;
            if (p < M) {
                i = ord[p];
                const bool held = D.flags && (D.flags[f * D.lcap + i] & 3) == 3;
                fresh = !held && D.ok[f * D.lcap + i];
                counts = held || fresh;
            }
            const unsigned long long b = __ballot(counts);
            const int before = run + __popcll(b & ((1ull << lane) - 1ull));
            if (fresh && before <= D.maxNew) { isNew[i] = 1; total++; }           // reached: no earlier `nLines > max_new_lines` break
            run += __popcll(b);
        }
    }
    __syncthreads();
    for (int i = lane; i < D.lcap; i += WAVE) D.isNew[f * D.lcap + i] = isNew[i];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) total += __shfl_xor(total, off);
    if (lane == 0) D.nNew[f] = total;
}

constexpr const char *WHO = "msl_lines_3d";

// line_flags is optional.
int check_line3d(int n_frames, int lcap, int order, const msl_line3d_params *params, const float *line_ends, const int32_t *n_lines, const float *depth,
                 size_t depth_row_stride, size_t depth_frame_stride, int width, int height, const uint8_t *, const float *Tcw, const uint32_t *seed,
                 msl_mem, float *line_depth, double *line_xyz, uint8_t *line_ok, uint8_t *line_new, int32_t *n_support, int32_t *n_new, msl_mem) {
    if (!none_null(WHO, {MSL_NAMED(params), MSL_NAMED(line_ends), MSL_NAMED(n_lines), MSL_NAMED(depth), MSL_NAMED(Tcw), MSL_NAMED(seed),
                         MSL_NAMED(line_depth), MSL_NAMED(line_xyz), MSL_NAMED(line_ok), MSL_NAMED(line_new), MSL_NAMED(n_support), MSL_NAMED(n_new)}))
        return MSL_ERR_INVALID;
    if (!at_least_one(WHO, "n_frames", n_frames)) return MSL_ERR_INVALID;
    if (lcap < 1 || lcap > MAX_KLCAP) { set_error("%s: lcap %d outside 1 .. %d", WHO, lcap, MAX_KLCAP); return MSL_ERR_INVALID; }
    if (order < MSL_LINE3D_ALL || order > MSL_LINE3D_DEPTH_ORDER) { set_error("%s: order %d is not an MSL_LINE3D_* value", WHO, order); return MSL_ERR_INVALID; }
    if (params->max_samples < 1 || params->max_samples > MAX_SAMPLES) {
        set_error("%s: max_samples %d outside 1 .. %d", WHO, params->max_samples, MAX_SAMPLES);
        return MSL_ERR_INVALID;
    }
    if (params->max_iterations < 0 || params->max_iterations > MAX_ITERS) {
        set_error("%s: max_iterations %d outside 0 .. %d", WHO, params->max_iterations, MAX_ITERS);
        return MSL_ERR_INVALID;
    }
    if (params->min_points < 2) { set_error("%s: min_points %d below 2", WHO, params->min_points); return MSL_ERR_INVALID; }
    if (width < 1 || height < 1 || depth_row_stride < (size_t)width * sizeof(float) || depth_row_stride % sizeof(float) != 0 ||
        depth_frame_stride % sizeof(float) != 0 || (n_frames > 1 && depth_frame_stride < depth_row_stride * (size_t)height)) {
        set_error("%s: depth image %d x %d with strides %zu / %zu bytes is not a float image", WHO, width, height, depth_row_stride,
                  depth_frame_stride);
        return MSL_ERR_INVALID;
    }
    return MSL_OK;
}

int launch_line3d(msl_match *h, int n_frames, int lcap, int order, const msl_line3d_params *prm, const float *line_ends, const int32_t *n_lines,
                  const float *depth, size_t depth_row_stride, size_t depth_frame_stride, int width, int height, const uint8_t *line_flags,
                  const float *Tcw, const uint32_t *seed, msl_mem mem, float *line_depth, double *line_xyz, uint8_t *line_ok, uint8_t *line_new,
                  int32_t *n_support, int32_t *n_new, msl_mem out_mem) {
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    hipStream_t st = h->stream;
    const size_t F = (size_t)n_frames, n = F * lcap;
    Line3dDev D{};
    D.lcap = lcap; D.order = order; D.width = width; D.height = height;
    D.fx = prm->fx; D.cx = prm->cx; D.cy = prm->cy; D.invfx = 1.0f / prm->fx; D.invfy = 1.0f / prm->fy;
    D.maxSamples = prm->max_samples; D.minPoints = prm->min_points; D.maxIter = prm->max_iterations; D.maxNew = prm->max_new_lines;
    D.distTh = prm->dist_thresh; D.minSupport = prm->min_support; D.minLength = prm->min_length;
    D.rowStride = depth_row_stride; D.frameStride = depth_frame_stride;
    MSL_HIP_TRY(h->line3d.grow(n * sizeof(LineDbg), st));
    D.dbg = (LineDbg *)h->line3d.p;
    h->line3dFrames = n_frames; h->line3dLcap = lcap;
    const size_t depthBytes = (F - 1) * depth_frame_stride + (size_t)(height - 1) * depth_row_stride + (size_t)width * sizeof(float);
    Stage S(h, mem, out_mem);
    D.ends = S.in(line_ends, 4 * n); D.nLines = S.in(n_lines, F); D.depth = S.in((const uint8_t *)depth, depthBytes);
    D.flags = S.in(line_flags, n); D.Tcw = S.in(Tcw, 12 * F); D.seed = S.in(seed, n);
    D.lineDepth = S.out(line_depth, 2 * n); D.xyz = S.out(line_xyz, 6 * n); D.ok = S.out(line_ok, n); D.isNew = S.out(line_new, n);
    D.nSupport = S.out(n_support, n); D.nNew = S.out(n_new, F);
    MSL_HIP_TRY(S.error());
    hipLaunchKernelGGL(k_line3d, dim3((unsigned)lcap, (unsigned)n_frames), dim3(WAVE), 0, st, D);
    MSL_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_line3d_select, dim3((unsigned)n_frames), dim3(WAVE), 0, st, D);
    MSL_HIP_TRY(hipGetLastError());
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}

}  // namespace

extern "C" {

int msl_lines_3d(msl_match *h, int n_frames, int lcap, int order, const msl_line3d_params *params, const float *line_ends,
                 const int32_t *n_lines, const float *depth, size_t depth_row_stride, size_t depth_frame_stride, int width, int height,
                 const uint8_t *line_flags, const float *Tcw, const uint32_t *seed, msl_mem mem, float *line_depth, double *line_xyz,
                 uint8_t *line_ok, uint8_t *line_new, int32_t *n_support, int32_t *n_new, msl_mem out_mem) noexcept {
    try {
    return handle_form(WHO, check_line3d, launch_line3d, h, n_frames, lcap, order, params, line_ends, n_lines, depth, depth_row_stride, depth_frame_stride,
                       width, height, line_flags, Tcw, seed, mem, line_depth, line_xyz, line_ok, line_new, n_support, n_new, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_lines_3d_batch(int device, int n_frames, int lcap, int order, const msl_line3d_params *params, const float *line_ends,
                       const int32_t *n_lines, const float *depth, size_t depth_row_stride, size_t depth_frame_stride, int width, int height,
                       const uint8_t *line_flags, const float *Tcw, const uint32_t *seed, msl_mem mem, float *line_depth, double *line_xyz,
                       uint8_t *line_ok, uint8_t *line_new, int32_t *n_support, int32_t *n_new, msl_mem out_mem) noexcept {
    try {
    return batch_form(check_line3d, launch_line3d, device, mem == MSL_MEM_DEVICE || out_mem == MSL_MEM_DEVICE, n_frames, lcap, order, params, line_ends,
                      n_lines, depth, depth_row_stride, depth_frame_stride, width, height, line_flags, Tcw, seed, mem, line_depth, line_xyz, line_ok, line_new,
                      n_support, n_new, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_lines_3d_debug(msl_match *h, int frame, int line, int32_t *counts, int32_t *iterations, double *md) noexcept {
    try {
    if (!h || !counts || !iterations || !md || frame < 0 || frame >= h->line3dFrames || line < 0 || line >= h->line3dLcap || !h->line3d.p) {
        set_error("msl_lines_3d_debug: invalid argument (keyline outside the last msl_lines_3d call?)");
        return MSL_ERR_INVALID;
    }
    std::vector<LineDbg> rec;
    int rc = last_call_row(h, h->line3d, (size_t)frame * h->line3dLcap + line, 1, rec);   // a row of one record
    if (rc != MSL_OK) return rc;
    const LineDbg &r = rec[0];
    counts[0] = r.nKept; counts[1] = r.nIter; counts[2] = r.refits; counts[3] = r.end[0]; counts[4] = r.end[1];
    for (int k = 0; k < MAX_ITERS; k++)
        for (int c = 0; c < 4; c++) iterations[4 * k + c] = k < r.nIter ? r.it[k][c] : 0;
    for (int i = 0; i < 3; i++) { md[i] = r.m[i]; md[3 + i] = r.d[i]; }
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}

}  // extern "C"

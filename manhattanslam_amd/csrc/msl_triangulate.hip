// msl_triangulate.hip -- batched LocalMapping::CreateNewMapPoints for gfx950 (reference src/LocalMapping.cc:303-522) with
// ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:257-406), CheckDistEpipolarLine (:127-144), LocalMapping::ComputeF12 (:624-640),
// KeyFrame::UnprojectStereo (src/KeyFrame.cc:544-557) and, for the two-observation point, MapPoint::UpdateNormalAndDepth
// (src/MapPoint.cc:282-322): msl_triangulate_new_points[_batch].
//
// Only the chain across an item's neighbours is ordered (a created point occupies its idx1 for the later neighbours), and it touches
// nothing but a taken flag per idx1 and the 30-bin rotation histogram.  Everything costly is computed for every (item, neighbour, idx1)
// from KF1's state on entry, whether or not an earlier neighbour will take that idx1:
//   k_tri_group    one workgroup per table keyframe: the searchable features (count, no map point, a node, a valid octave, stereo when
//                  only_stereo) as (node << 13 | index) keys, sorted in LDS (the bitonic sort of msl_match_by_bow) -> the FeatureVector
//   k_tri_pair     one thread per (item, neighbour): Ow of both, the baseline test, F12, the epipole
//   k_tri_search   one wave per (item, neighbour, idx1): lower bound of idx1's node in KF2's keys, the node's KF2 features over the lanes,
//                  popcount distance, epipole exclusion, epipolar line; minimum of (dist << 13 | 8191 - idx2) = smallest distance, the
//                  later idx2 on ties; -> candidate idx2 and rotation bin
//   k_tri_verdict  one lane per candidate: parallax, the 4x4 solve or UnprojectStereo, depth, reprojection and scale tests, the point's
//                  normal and distances -> status code and point
//   k_tri_walk     one wave per item, its neighbours in order: live = candidates whose idx1 is not taken; histogram, three maxima, cull;
//                  match12 / nmatches / status; created = kept and verdict ok -> the point outputs and new_order (ballot prefix rank,
//                  ascending idx1); taken |= created
//
// Pins (tests/triangulate_model.py is the sequential model and the kernels run its
// operations in its order, contraction off):
//   * cv::Mat products: gemm3's rule (double products and the + t term accumulated in double, one rounding to float)
//   * Mat::dot, cv::norm: double accumulation in index order, sqrt in double, rounded where the reference assigns to float
//   * F12: M = -(R1w R2w^T) one gemm (alpha = -1), t12 = M t2w + t1w one gemm, K.t().inv() and K.inv() by the closed 3x3 form (determinant
//     and cofactors in double, times 1 / det, each element rounded), then the three products left to right
//   * comparisons against double literals (3.84, 5.991, 7.8, 0.9998) in double on the float operands; 100 * scaleFactor in float
//   * cos(2 atan2(b / 2, depth)) = (d^2 - a^2) / (d^2 + a^2), a = b / 2 in float, the quotient in double, rounded to float
//   * rows of A: a float multiply, then a float subtract
//   * cv::SVD: the cyclic Jacobi eigen-solver of msl_jacobi.h (jacobi_sweep<4>: 16 sweeps, round-robin steps {(0,3),(1,2)}, {(1,3),(0,2)},
//     {(2,3),(0,1)}, the angles of a step from the matrix before it, rows then columns) on A^T A in double (sums over the rows of A in order); vt.row(3) =
//     the eigenvector of the smallest eigenvalue (the highest index on ties) cast to float; then == 0 on its fourth component and a float
//     division
//   * invz = (float)(1.0 / z); u = fx * x * invz + cx in float, left to right
//   * normali / cv::norm(normali) = (float)((double)x * (1.0 / norm)); the float sum of the two terms; then * 0.5
//   * UnprojectStereo of a stereo keypoint with depth <= 0 (an empty Mat in the reference): rejected as low parallax
//   * a keypoint whose octave is outside [0, nlevels) is never searched, on either side
//   * a table index outside [0, n_tab), or a neighbour equal to the current keyframe, that only the device can see: that neighbour is
//     skipped (an invalid current keyframe has no keypoints)
#include "msl_jacobi.h"
#include "msl_index_check.h"
#include "msl_match_handle.h"
#include "msl_match_math.h"

#include <vector>

namespace {

using namespace msl;

constexpr int MAX_NCAP = 16, IDX_BITS = 13;
constexpr int GROUP_NT = 1024, SEARCH_NT = 256, VERDICT_NT = 64;
constexpr unsigned long long KEY_NONE = ~0ull;

// What the geometry kernel leaves per (item, neighbour); msl_debug_triangulate reads F12, ex, ey, baseline.
struct TriPair {
    float F12[9], ex, ey, baseline;
    float Ow1[3], Ow2[3];
    int32_t k1, k2, skip, pad;                     // table indices (-1: invalid); skip: baseline < b, or an invalid pair
};

// What the search and the verdict leave per (item, neighbour, idx1).
struct TriRec {
    int32_t idx2, bin, status;                     // idx2 -1: no candidate
    float cosRays, cos1, cos2, x3D[4];
    float xyz[3], normal[3], dist[2];
};

struct TriDev {
    int nTab, cap, nItems, ncap, P;
    msl_triangulate_params prm;
    const msl_keypoint *kps; const float *raw, *uright, *depth; const uint8_t *desc; const int32_t *node; const uint8_t *held;
    const int32_t *n; const float *Tcw;
    const int32_t *cur, *neigh, *nNeigh;
    int32_t *match12; uint8_t *status; int32_t *nmatches, *newNeigh, *newIdx2; float *newXyz, *newNormal, *newDist; uint8_t *newDesc;
    int32_t *newOrder, *nNew;
    unsigned long long *keys; TriPair *pair; TriRec *rec;
};

__device__ __forceinline__ bool octave_ok(const TriDev &D, int o) { return o >= 0 && o < D.prm.nlevels; }

// ==== the FeatureVector of every table keyframe ==============================================================================================
__global__ __launch_bounds__(GROUP_NT) void k_tri_group(TriDev D) {
    extern __shared__ unsigned long long s_key[];
    const int k = blockIdx.x, P = D.P;
    const int n = clampi(D.n[k], 0, D.cap);
    const size_t base = (size_t)k * D.cap;
    for (int i = threadIdx.x; i < P; i += GROUP_NT) {
        unsigned long long key = KEY_NONE;
        if (i < n) {
            const int nd = D.node[base + i];
            const bool ok = nd >= 0 && !D.held[base + i] && octave_ok(D, D.kps[base + i].octave) &&
                            (!D.prm.only_stereo || D.uright[base + i] >= 0);
            if (ok) key = ((unsigned long long)(unsigned)nd << IDX_BITS) | (unsigned)i;
        }
        s_key[i] = key;
    }
    bitonic_sort(s_key, P);
    for (int i = threadIdx.x; i < P; i += GROUP_NT) D.keys[(size_t)k * P + i] = s_key[i];
}

// ==== pair geometry ==========================================================================================================================
__global__ __launch_bounds__(64) void k_tri_pair(TriDev D) {
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= D.nItems * D.ncap) return;
    const int f = g / D.ncap, r = g - f * D.ncap;
    TriPair G{};
    G.k1 = G.k2 = -1; G.skip = 1;
    const int nn = clampi(D.nNeigh[f], 0, D.ncap);
    const int k1 = D.cur[f];
    if (k1 >= 0 && k1 < D.nTab) G.k1 = k1;
    if (r < nn) {
        const int k2 = D.neigh[g];
        if (k2 >= 0 && k2 < D.nTab && k2 != k1) G.k2 = k2;
    }
    if (G.k1 >= 0 && G.k2 >= 0) {
        const float *T1 = D.Tcw + (size_t)G.k1 * 12, *T2 = D.Tcw + (size_t)G.k2 * 12;
        camera_centre(T1, G.Ow1); camera_centre(T2, G.Ow2);
        const float vb[3] = {G.Ow2[0] - G.Ow1[0], G.Ow2[1] - G.Ow1[1], G.Ow2[2] - G.Ow1[2]};
        G.baseline = (float)norm3_dacc(vb);
        G.skip = G.baseline < D.prm.b ? 1 : 0;
        // ComputeF12
        const float t1w[3] = {T1[3], T1[7], T1[11]}, t2w[3] = {T2[3], T2[7], T2[11]};
        float R12[9], M[9], t12[3];
        gemm33<4, 4>(T1, false, T2, true, 1.0, R12);
        gemm33<4, 4>(T1, false, T2, true, -1.0, M);
        gemm3<3>(M, false, 1.0, t2w, t1w, t12);
        const float t12x[9] = {0.0f, -t12[2], t12[1], t12[2], 0.0f, -t12[0], -t12[1], t12[0], 0.0f};
        const float K[9] = {D.prm.fx, 0.0f, D.prm.cx, 0.0f, D.prm.fy, D.prm.cy, 0.0f, 0.0f, 1.0f};
        const float Kt[9] = {D.prm.fx, 0.0f, 0.0f, 0.0f, D.prm.fy, 0.0f, D.prm.cx, D.prm.cy, 1.0f};
        float Kti[9], Ki[9], a[9], b[9];
        inv33(Kt, Kti); inv33(K, Ki);
        gemm33<3, 3>(Kti, false, t12x, false, 1.0, a);
        gemm33<3, 3>(a, false, R12, false, 1.0, b);
        gemm33<3, 3>(b, false, Ki, false, 1.0, G.F12);
        // the epipole in the second image
        float C2[3];
        gemm3(T2, false, 1.0, G.Ow1, t2w, C2);
        const float invz = 1.0f / C2[2];
        G.ex = D.prm.fx * C2[0] * invz + D.prm.cx;
        G.ey = D.prm.fy * C2[1] * invz + D.prm.cy;
    }
    D.pair[g] = G;
}

// ==== candidate search =======================================================================================================================
__global__ __launch_bounds__(SEARCH_NT) void k_tri_search(TriDev D) {
    const int f = blockIdx.z, r = blockIdx.y, lane = lane_id();
    const int idx1 = blockIdx.x * (SEARCH_NT / 64) + (threadIdx.x >> 6);
    if (idx1 >= D.cap) return;                                                 // uniform per wave
    const size_t pr = (size_t)f * D.ncap + r;
    TriRec *out = D.rec + pr * D.cap + idx1;
    const TriPair &G = D.pair[pr];
    int best = -1, bin = -1;
    if (!G.skip) {
        const size_t b1 = (size_t)G.k1 * D.cap, b2 = (size_t)G.k2 * D.cap;
        const int n1 = clampi(D.n[G.k1], 0, D.cap);
        bool ok = idx1 < n1;
        int nd = -1;
        float ur1 = -1.0f;
        msl_keypoint kp1{};
        if (ok) {
            nd = D.node[b1 + idx1]; ur1 = D.uright[b1 + idx1]; kp1 = D.kps[b1 + idx1];
            ok = nd >= 0 && !D.held[b1 + idx1] && octave_ok(D, kp1.octave) && (!D.prm.only_stereo || ur1 >= 0);
        }
        if (ok) {                                                              // uniform: every lane read the same values
            const bool stereo1 = ur1 >= 0;
            const unsigned long long *keys = D.keys + (size_t)G.k2 * D.P;
            const unsigned long long want = (unsigned long long)(unsigned)nd << IDX_BITS;
            int lo = 0, hi = D.P;                                              // lower_bound of the node in KF2's keys
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (keys[mid] < want) lo = mid + 1; else hi = mid; }
            // the epipolar line of kp1 in the second image: l = x1' F12 = [a b c]
            const float *F = G.F12;
            const float a = kp1.x * F[0] + kp1.y * F[3] + F[6];
            const float b = kp1.x * F[1] + kp1.y * F[4] + F[7];
            const float c = kp1.x * F[2] + kp1.y * F[5] + F[8];
            const float den = a * a + b * b;
            uint4 d0, d1;
            load_desc(D.desc + (b1 + idx1) * 32, d0, d1);
            unsigned key = 0xFFFFFFFFu;
            for (int at = lo;; at += 64) {
                const int p = at + lane;
                const unsigned long long k2 = p < D.P ? keys[p] : KEY_NONE;
                const bool in = (k2 >> IDX_BITS) == (unsigned long long)(unsigned)nd;   // KEY_NONE >> 13 is above every node
                if (in) {
                    const int idx2 = (int)(k2 & (MAX_CAP - 1));
                    uint4 e0, e1;
                    load_desc(D.desc + (b2 + idx2) * 32, e0, e1);
                    const int dist = hamming256(d0, d1, e0, e1);
                    if (dist <= TH_LOW) {
                        const msl_keypoint kp2 = D.kps[b2 + idx2];
                        bool pass = true;
                        if (!stereo1 && !(D.uright[b2 + idx2] >= 0)) {
                            const float distex = G.ex - kp2.x, distey = G.ey - kp2.y;
                            if (distex * distex + distey * distey < 100 * D.prm.scale_factors[kp2.octave]) pass = false;
                        }
                        if (pass) {                                            // CheckDistEpipolarLine
                            const float num = a * kp2.x + b * kp2.y + c;
                            if (den == 0) pass = false;
                            else {
                                const float dsqr = num * num / den;
                                pass = (double)dsqr < 3.84 * (double)D.prm.level_sigma2[kp2.octave];
                            }
                        }
                        if (pass) { const unsigned kk = ((unsigned)dist << IDX_BITS) | (unsigned)(MAX_CAP - 1 - idx2); key = kk < key ? kk : key; }
                    }
                }
                if (__ballot(in) != ~0ull) break;                              // the node's run ended inside this chunk
            }
            key = wave_min(key);
            if (key != 0xFFFFFFFFu) {
                best = MAX_CAP - 1 - (int)(key & (MAX_CAP - 1));
                bin = rot_bin(kp1.angle - D.kps[b2 + best].angle);
            }
        }
    }
    if (lane == 0) { out->idx2 = best; out->bin = bin; out->status = MSL_TRI_NO_MATCH; }
}

// ==== triangulation verdict ==================================================================================================================
// vt.row(3) of cv::SVD of the 4x4 float A (rows r0..r3), pinned: the eigenvector of the smallest eigenvalue of A^T A, cast to float
__device__ __forceinline__ void null_vector(const float (&Am)[16], float x[4]) {
    double G[16], V[16];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 4; k++) s = s + (double)Am[k * 4 + i] * (double)Am[k * 4 + j];
            G[i * 4 + j] = s;
            V[i * 4 + j] = i == j ? 1.0 : 0.0;
        }
#pragma unroll 1
    for (int sw = 0; sw < JACOBI_SWEEPS; sw++) jacobi_sweep<4>(G, V);
    // descending order with the lower index first on ties: the last is the smallest, the highest index among equals
    int m = 0; double dm = G[0];
    if (G[5] <= dm) { dm = G[5]; m = 1; }
    if (G[10] <= dm) { dm = G[10]; m = 2; }
    if (G[15] <= dm) { dm = G[15]; m = 3; }
#pragma unroll
    for (int a = 0; a < 4; a++) x[a] = (float)(m == 0 ? V[a * 4] : m == 1 ? V[a * 4 + 1] : m == 2 ? V[a * 4 + 2] : V[a * 4 + 3]);
}

// cos(2 atan2(b / 2, depth)), pinned to its closed form
__device__ __forceinline__ float cos_stereo(float b, float depth) {
    const float a = b / 2;
    const double a2 = (double)a * (double)a, d2 = (double)depth * (double)depth;
    return (float)((d2 - a2) / (d2 + a2));
}

// KeyFrame::UnprojectStereo; false: depth <= 0
__device__ __forceinline__ bool unproject(const TriDev &D, const float *T, const float Ow[3], float u, float v, float z, float X[3]) {
    if (!(z > 0)) return false;
    const float x = (u - D.prm.cx) * z * D.prm.invfx, y = (v - D.prm.cy) * z * D.prm.invfy;
    const float pc[3] = {x, y, z};
    gemm3(T, true, 1.0, pc, Ow, X);                                            // Twc(0:3, 0:3) * x3Dc + Twc(0:3, 3)
    return true;
}

// The reprojection test of one keyframe for a point at depth z > 0 in it: true = the error is above the chi-square bound
__device__ __forceinline__ bool reproj_bad(const msl_triangulate_params &K, const float *T, const float X[3], float z, const msl_keypoint &kp,
                                           float ur, bool stereo) {
    const float sigma2 = K.level_sigma2[kp.octave];
    const float x = (float)(dot3_dacc(T, X) + (double)T[3]), y = (float)(dot3_dacc(T + 4, X) + (double)T[7]);
    const float invz = (float)(1.0 / (double)z);
    const float u = K.fx * x * invz + K.cx, v = K.fy * y * invz + K.cy;
    const float errX = u - kp.x, errY = v - kp.y;
    if (!stereo) return (double)(errX * errX + errY * errY) > 5.991 * (double)sigma2;
    const float u_r = u - K.bf * invz, errXr = u_r - ur;
    return (double)(errX * errX + errY * errY + errXr * errXr) > 7.8 * (double)sigma2;
}

__global__ __launch_bounds__(VERDICT_NT) void k_tri_verdict(TriDev D) {
    const int f = blockIdx.z, r = blockIdx.y;
    const int idx1 = blockIdx.x * VERDICT_NT + threadIdx.x;
    if (idx1 >= D.cap) return;
    const size_t pr = (size_t)f * D.ncap + r;
    TriRec &R = D.rec[pr * D.cap + idx1];
    const int idx2 = R.idx2;
    if (idx2 < 0) return;
    const TriPair &G = D.pair[pr];
    const msl_triangulate_params &K = D.prm;
    const size_t i1 = (size_t)G.k1 * D.cap + idx1, i2 = (size_t)G.k2 * D.cap + idx2;
    const float *T1 = D.Tcw + (size_t)G.k1 * 12, *T2 = D.Tcw + (size_t)G.k2 * 12;
    const msl_keypoint kp1 = D.kps[i1], kp2 = D.kps[i2];
    const float ur1 = D.uright[i1], ur2 = D.uright[i2];
    const bool s1 = ur1 >= 0, s2 = ur2 >= 0;
    // parallax between the rays
    const float xn1[3] = {(kp1.x - K.cx) * K.invfx, (kp1.y - K.cy) * K.invfy, 1.0f};
    const float xn2[3] = {(kp2.x - K.cx) * K.invfx, (kp2.y - K.cy) * K.invfy, 1.0f};
    float ray1[3], ray2[3];
    gemm3(T1, true, 1.0, xn1, nullptr, ray1);
    gemm3(T2, true, 1.0, xn2, nullptr, ray2);
    const float cosRays = (float)(dot3_dacc(ray1, ray2) / (norm3_dacc(ray1) * norm3_dacc(ray2)));
    float cosStereo = cosRays + 1;
    float cos1 = cosStereo, cos2 = cosStereo;
    if (s1) cos1 = cos_stereo(K.b, D.depth[i1]);
    else if (s2) cos2 = cos_stereo(K.b, D.depth[i2]);
    cosStereo = cos2 < cos1 ? cos2 : cos1;                                     // std::min
    float x4[4] = {0.0f, 0.0f, 0.0f, 0.0f}, X[3] = {0.0f, 0.0f, 0.0f};
    int status = MSL_TRI_NO_MATCH;
    if (cosRays < cosStereo && cosRays > 0 && (s1 || s2 || (double)cosRays < 0.9998)) {
        float A[16];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            A[j] = xn1[0] * T1[8 + j] - T1[j];
            A[4 + j] = xn1[1] * T1[8 + j] - T1[4 + j];
            A[8 + j] = xn2[0] * T2[8 + j] - T2[j];
            A[12 + j] = xn2[1] * T2[8 + j] - T2[4 + j];
        }
        null_vector(A, x4);
        if (x4[3] == 0) status = MSL_TRI_W_ZERO;
        else { X[0] = x4[0] / x4[3]; X[1] = x4[1] / x4[3]; X[2] = x4[2] / x4[3]; status = MSL_TRI_TRIANGULATED; }
    } else if (s1 && cos1 < cos2) {
        status = unproject(D, T1, G.Ow1, D.raw[2 * i1], D.raw[2 * i1 + 1], D.depth[i1], X) ? MSL_TRI_STEREO1 : MSL_TRI_LOW_PARALLAX;
    } else if (s2 && cos2 < cos1) {
        status = unproject(D, T2, G.Ow2, D.raw[2 * i2], D.raw[2 * i2 + 1], D.depth[i2], X) ? MSL_TRI_STEREO2 : MSL_TRI_LOW_PARALLAX;
    } else {
        status = MSL_TRI_LOW_PARALLAX;
    }
    float normal[3] = {0.0f, 0.0f, 0.0f}, dist[2] = {0.0f, 0.0f};
    if (status >= MSL_TRI_TRIANGULATED && status <= MSL_TRI_STEREO2) {
        const int made = status;
        // in front of both cameras, then the reprojection error in each
        const float z1 = (float)(dot3_dacc(T1 + 8, X) + (double)T1[11]);
        if (z1 <= 0) status = MSL_TRI_Z1;
        else {
            const float z2 = (float)(dot3_dacc(T2 + 8, X) + (double)T2[11]);
            if (z2 <= 0) status = MSL_TRI_Z2;
            else if (reproj_bad(K, T1, X, z1, kp1, ur1, s1)) status = MSL_TRI_REPROJ1;
            else if (reproj_bad(K, T2, X, z2, kp2, ur2, s2)) status = MSL_TRI_REPROJ2;
        }
        if (status == made) {
            const float n1v[3] = {X[0] - G.Ow1[0], X[1] - G.Ow1[1], X[2] - G.Ow1[2]}, n2v[3] = {X[0] - G.Ow2[0], X[1] - G.Ow2[1], X[2] - G.Ow2[2]};
            const double nd1 = norm3_dacc(n1v), nd2 = norm3_dacc(n2v);
            const float dist1 = (float)nd1, dist2 = (float)nd2;
            if (dist1 == 0 || dist2 == 0) status = MSL_TRI_ZERO_DIST;
            else {
                const float ratioDist = dist2 / dist1, ratioFactor = 1.5f * K.scale_factor;
                const float ratioOctave = K.scale_factors[kp1.octave] / K.scale_factors[kp2.octave];
                if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) status = MSL_TRI_SCALE;
                else {
                    // UpdateNormalAndDepth with the observations (KF2, KF1) and KF1 as reference keyframe
                    const double i1n = 1.0 / nd1, i2n = 1.0 / nd2;
#pragma unroll
                    for (int a = 0; a < 3; a++) {
                        float acc = 0.0f + (float)((double)n2v[a] * i2n);
                        acc = acc + (float)((double)n1v[a] * i1n);
                        normal[a] = (float)((double)acc * 0.5);
                    }
                    dist[1] = dist1 * K.scale_factors[kp1.octave];
                    dist[0] = dist[1] / K.scale_factors[K.nlevels - 1];
                }
            }
        }
    }
    R.status = status; R.cosRays = cosRays; R.cos1 = cos1; R.cos2 = cos2;
#pragma unroll
    for (int a = 0; a < 4; a++) R.x3D[a] = x4[a];
#pragma unroll
    for (int a = 0; a < 3; a++) { R.xyz[a] = X[a]; R.normal[a] = normal[a]; }
    R.dist[0] = dist[0]; R.dist[1] = dist[1];
}

// ==== the ordered walk =======================================================================================================================
__global__ __launch_bounds__(WAVE) void k_tri_walk(TriDev D) {
    __shared__ uint8_t s_taken[MAX_CAP];                                       // entry i is read and written by lane i % 64 only
    __shared__ int s_hist[ROT_HISTO_LENGTH];
    const int f = blockIdx.x, lane = threadIdx.x, cap = D.cap;
    const TriPair *pairs = D.pair + (size_t)f * D.ncap;
    const int k1 = pairs[0].k1;
    const int n1 = k1 >= 0 ? clampi(D.n[k1], 0, cap) : 0;
    const int nn = clampi(D.nNeigh[f], 0, D.ncap);
    const size_t fb = (size_t)f * cap;
    for (int i = lane; i < cap; i += WAVE) {
        s_taken[i] = 0;
        D.newNeigh[fb + i] = -1; D.newIdx2[fb + i] = -1;
        for (int a = 0; a < 3; a++) { D.newXyz[3 * (fb + i) + a] = 0.0f; D.newNormal[3 * (fb + i) + a] = 0.0f; }
        D.newDist[2 * (fb + i)] = 0.0f; D.newDist[2 * (fb + i) + 1] = 0.0f;
        uint4 *dd = reinterpret_cast<uint4 *>(D.newDesc + (fb + i) * 32);
        dd[0] = make_uint4(0, 0, 0, 0); dd[1] = make_uint4(0, 0, 0, 0);
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    int nNew = 0;
    for (int r = 0; r < D.ncap; r++) {
        const size_t pb = ((size_t)f * D.ncap + r) * cap;
        const bool active = r < nn && !pairs[r].skip;
        if (!active) {                                                         // a skipped neighbour changes nothing
            const uint8_t st = r < nn ? MSL_TRI_NEIGHBOUR_SKIPPED : MSL_TRI_NO_MATCH;
            for (int i = lane; i < cap; i += WAVE) { D.match12[pb + i] = -1; D.status[pb + i] = i < n1 ? st : (uint8_t)MSL_TRI_NO_MATCH; }
            if (lane == 0) D.nmatches[(size_t)f * D.ncap + r] = 0;
            continue;
        }
        const TriRec *rec = D.rec + pb;
        int keep[3] = {-1, -1, -1};
        if (D.prm.check_orientation) {
            __syncthreads();
            if (lane < ROT_HISTO_LENGTH) s_hist[lane] = 0;
            __syncthreads();
            for (int i = lane; i < n1; i += WAVE) {
                const int b = rec[i].bin;
                if (rec[i].idx2 >= 0 && !s_taken[i] && b >= 0) atomicAdd(&s_hist[b], 1);
            }
            __syncthreads();
            three_maxima(s_hist, keep);
        }
        int nm = 0;
        const size_t b2 = (size_t)pairs[r].k2 * cap;
        for (int at = 0; at < cap; at += WAVE) {
            const int i = at + lane;
            int idx2 = -1, st = MSL_TRI_NO_MATCH;
            if (i < n1 && !s_taken[i]) {
                idx2 = rec[i].idx2;
                const int b = rec[i].bin;
                if (idx2 >= 0 && D.prm.check_orientation && b >= 0 && b != keep[0] && b != keep[1] && b != keep[2]) idx2 = -1;
                if (idx2 >= 0) st = rec[i].status;
            }
            if (i < cap) { D.match12[pb + i] = idx2; D.status[pb + i] = (uint8_t)st; }
            nm += __popcll(__ballot(idx2 >= 0));
            const bool made = idx2 >= 0 && st >= MSL_TRI_TRIANGULATED && st <= MSL_TRI_STEREO2;
            const unsigned long long mb = __ballot(made);
            if (made) {
                const int rank = nNew + __popcll(mb & below);
                D.newOrder[fb + rank] = i;
                D.newNeigh[fb + i] = r; D.newIdx2[fb + i] = idx2;
                for (int a = 0; a < 3; a++) { D.newXyz[3 * (fb + i) + a] = rec[i].xyz[a]; D.newNormal[3 * (fb + i) + a] = rec[i].normal[a]; }
                D.newDist[2 * (fb + i)] = rec[i].dist[0]; D.newDist[2 * (fb + i) + 1] = rec[i].dist[1];
                // ComputeDistinctiveDescriptors with two observations: the first in creation order, the older keyframe KF2
                const uint4 *sd = reinterpret_cast<const uint4 *>(D.desc + (b2 + idx2) * 32);
                uint4 *dd = reinterpret_cast<uint4 *>(D.newDesc + (fb + i) * 32);
                dd[0] = sd[0]; dd[1] = sd[1];
                s_taken[i] = 1;                                                // AddMapPoint(pMP, idx1)
            }
            nNew += __popcll(mb);
        }
        if (lane == 0) D.nmatches[(size_t)f * D.ncap + r] = nm;
    }
    for (int j = nNew + lane; j < cap; j += WAVE) D.newOrder[fb + j] = -1;
    if (lane == 0) D.nNew[f] = nNew;
}

// ==== host side ==============================================================================================================================
const char *const WHO_TRI = "msl_triangulate_new_points";

int check_triangulate(int n_tab, int cap, int n_items, int ncap, const msl_triangulate_params *params, const msl_keypoint *kps_un,
                      const float *raw_xy, const float *uright, const float *depth, const uint8_t *desc, const int32_t *node, const uint8_t *held,
                      const int32_t *n_kps, const float *Tcw, const int32_t *cur, const int32_t *neigh, const int32_t *n_neigh, msl_mem mem,
                      int32_t *match12, uint8_t *status, int32_t *nmatches, int32_t *new_neigh, int32_t *new_idx2, float *new_xyz,
                      float *new_normal, float *new_dist, uint8_t *new_desc, int32_t *new_order, int32_t *n_new, msl_mem) {
    const char *who = WHO_TRI;
    if (!none_null(who, {MSL_NAMED(params), MSL_NAMED(kps_un), MSL_NAMED(raw_xy), MSL_NAMED(uright), MSL_NAMED(depth), MSL_NAMED(desc),
                         MSL_NAMED(node), MSL_NAMED(held), MSL_NAMED(n_kps), MSL_NAMED(Tcw), MSL_NAMED(cur), MSL_NAMED(neigh), MSL_NAMED(n_neigh),
                         MSL_NAMED(match12), MSL_NAMED(status), MSL_NAMED(nmatches), MSL_NAMED(new_neigh), MSL_NAMED(new_idx2), MSL_NAMED(new_xyz),
                         MSL_NAMED(new_normal), MSL_NAMED(new_dist), MSL_NAMED(new_desc), MSL_NAMED(new_order), MSL_NAMED(n_new)}))
        return MSL_ERR_INVALID;
    if (n_tab < 1 || n_tab > MAX_TAB) { set_error("%s: n_tab %d outside 1 .. %d", who, n_tab, MAX_TAB); return MSL_ERR_INVALID; }
    if (n_items < 1) { set_error("%s: n_items %d below 1", who, n_items); return MSL_ERR_INVALID; }
    if (cap < 1 || cap > MAX_CAP) { set_error("%s: cap %d outside 1 .. %d", who, cap, MAX_CAP); return MSL_ERR_INVALID; }
    if (ncap < 1 || ncap > MAX_NCAP) { set_error("%s: ncap %d outside 1 .. %d", who, ncap, MAX_NCAP); return MSL_ERR_INVALID; }
    if (n_items > 65535) { set_error("%s: n_items %d above 65535", who, n_items); return MSL_ERR_INVALID; }
    if (!levels_ok(who, params->nlevels)) return MSL_ERR_INVALID;
    char why[256];
    if (mem == MSL_MEM_HOST && !check::neighbours_ok(n_tab, n_items, ncap, cur, neigh, n_neigh, why, sizeof(why))) return refuse(who, why);
    return MSL_OK;
}

int launch_triangulate(msl_match *h, int n_tab, int cap, int n_items, int ncap, const msl_triangulate_params *prm, const msl_keypoint *kps_un,
                       const float *raw_xy, const float *uright, const float *depth, const uint8_t *desc, const int32_t *node, const uint8_t *held,
                       const int32_t *n_kps, const float *Tcw, const int32_t *cur, const int32_t *neigh, const int32_t *n_neigh, msl_mem mem,
                       int32_t *match12, uint8_t *status, int32_t *nmatches, int32_t *new_neigh, int32_t *new_idx2, float *new_xyz,
                       float *new_normal, float *new_dist, uint8_t *new_desc, int32_t *new_order, int32_t *n_new, msl_mem out_mem) {
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    hipStream_t st = h->stream;
    const size_t T = (size_t)n_tab, nt = T * cap, F = (size_t)n_items, np = F * ncap, nf = F * cap, nr = np * cap;
    TriDev D{};
    D.nTab = n_tab; D.cap = cap; D.nItems = n_items; D.ncap = ncap; D.P = pow2_at_least(cap > 2 ? cap : 2);
    D.prm = *prm;
    MSL_HIP_TRY(grow_all(st, {{h->triKeys, T * D.P * sizeof(unsigned long long)}, {h->triPair, np * sizeof(TriPair)}, {h->triRec, nr * sizeof(TriRec)}}));
    D.keys = (unsigned long long *)h->triKeys.p; D.pair = (TriPair *)h->triPair.p; D.rec = (TriRec *)h->triRec.p;
    h->triItems = n_items; h->triNcap = ncap; h->triCap = cap;
    Stage S(h, mem, out_mem);
    D.kps = S.in(kps_un, nt); D.raw = S.in(raw_xy, 2 * nt); D.uright = S.in(uright, nt); D.depth = S.in(depth, nt); D.desc = S.in(desc, 32 * nt);
    D.node = S.in(node, nt); D.held = S.in(held, nt); D.n = S.in(n_kps, T); D.Tcw = S.in(Tcw, 12 * T);
    D.cur = S.in(cur, F); D.neigh = S.in(neigh, np); D.nNeigh = S.in(n_neigh, F);
    D.match12 = S.out(match12, nr); D.status = S.out(status, nr); D.nmatches = S.out(nmatches, np);
    D.newNeigh = S.out(new_neigh, nf); D.newIdx2 = S.out(new_idx2, nf); D.newXyz = S.out(new_xyz, 3 * nf); D.newNormal = S.out(new_normal, 3 * nf);
    D.newDist = S.out(new_dist, 2 * nf); D.newDesc = S.out(new_desc, 32 * nf); D.newOrder = S.out(new_order, nf); D.nNew = S.out(n_new, F);
    MSL_HIP_TRY(S.error());
    MSL_HIP_TRY(allow_lds(h, LDS_TRI_GROUP, k_tri_group, 8 * MAX_CAP));
    hipLaunchKernelGGL(k_tri_group, dim3((unsigned)n_tab), dim3(GROUP_NT), 8 * (size_t)D.P, st, D);
    MSL_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_tri_pair, dim3((unsigned)((np + 63) / 64)), dim3(64), 0, st, D);
    MSL_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_tri_search, dim3((unsigned)((cap + SEARCH_NT / 64 - 1) / (SEARCH_NT / 64)), (unsigned)ncap, (unsigned)n_items), dim3(SEARCH_NT),
                       0, st, D);
    MSL_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_tri_verdict, dim3((unsigned)((cap + VERDICT_NT - 1) / VERDICT_NT), (unsigned)ncap, (unsigned)n_items), dim3(VERDICT_NT), 0, st,
                       D);
    MSL_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_tri_walk, dim3((unsigned)n_items), dim3(WAVE), 0, st, D);
    MSL_HIP_TRY(hipGetLastError());
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}

}  // namespace

extern "C" {

int msl_triangulate_new_points(msl_match *h, int n_tab, int cap, int n_items, int ncap, const msl_triangulate_params *params,
                               const msl_keypoint *kps_un, const float *raw_xy, const float *uright, const float *depth, const uint8_t *desc,
                               const int32_t *node, const uint8_t *held, const int32_t *n_kps, const float *Tcw, const int32_t *cur,
                               const int32_t *neigh, const int32_t *n_neigh, msl_mem mem, int32_t *match12, uint8_t *status, int32_t *nmatches,
                               int32_t *new_neigh, int32_t *new_idx2, float *new_xyz, float *new_normal, float *new_dist, uint8_t *new_desc,
                               int32_t *new_order, int32_t *n_new, msl_mem out_mem) noexcept {
    try {
    return handle_form(WHO_TRI, check_triangulate, launch_triangulate, h, n_tab, cap, n_items, ncap, params, kps_un, raw_xy, uright, depth, desc, node,
                       held, n_kps, Tcw, cur, neigh, n_neigh, mem, match12, status, nmatches, new_neigh, new_idx2, new_xyz, new_normal, new_dist,
                       new_desc, new_order, n_new, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_triangulate_new_points_batch(int device, int n_tab, int cap, int n_items, int ncap, const msl_triangulate_params *params,
                                     const msl_keypoint *kps_un, const float *raw_xy, const float *uright, const float *depth, const uint8_t *desc,
                                     const int32_t *node, const uint8_t *held, const int32_t *n_kps, const float *Tcw, const int32_t *cur,
                                     const int32_t *neigh, const int32_t *n_neigh, msl_mem mem, int32_t *match12, uint8_t *status,
                                     int32_t *nmatches, int32_t *new_neigh, int32_t *new_idx2, float *new_xyz, float *new_normal, float *new_dist,
                                     uint8_t *new_desc, int32_t *new_order, int32_t *n_new, msl_mem out_mem) noexcept {
    try {
    return batch_form(check_triangulate, launch_triangulate, device, mem == MSL_MEM_DEVICE, n_tab, cap, n_items, ncap, params, kps_un, raw_xy, uright,
                      depth, desc, node, held, n_kps, Tcw, cur, neigh, n_neigh, mem, match12, status, nmatches, new_neigh, new_idx2, new_xyz, new_normal,
                      new_dist, new_desc, new_order, n_new, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_debug_triangulate(msl_match *h, int item, int neigh, float *pair, int32_t *cand, float *cosines, float *x3d) noexcept {
    try {
    if (!h || !pair || !cand || !cosines || !x3d || item < 0 || item >= h->triItems || neigh < 0 || neigh >= h->triNcap || !h->triRec.p) {
        set_error("msl_debug_triangulate: invalid argument (pair outside the last msl_triangulate_new_points call?)");
        return MSL_ERR_INVALID;
    }
    const size_t pr = (size_t)item * h->triNcap + neigh;
    TriPair G;
    std::vector<TriRec> rec;
    int rc = last_call_row(h, h->triRec, pr, (size_t)h->triCap, rec);
    if (rc != MSL_OK) return rc;
    MSL_HIP_TRY(hipMemcpy(&G, (const TriPair *)h->triPair.p + pr, sizeof(TriPair), hipMemcpyDeviceToHost));
    for (int i = 0; i < 9; i++) pair[i] = G.F12[i];
    pair[9] = G.ex; pair[10] = G.ey; pair[11] = G.baseline;
    for (int i = 0; i < h->triCap; i++) {
        const TriRec &r = rec[(size_t)i];
        const bool has = r.idx2 >= 0;
        cand[2 * i] = r.idx2; cand[2 * i + 1] = has ? r.bin : -1;
        cosines[3 * i] = has ? r.cosRays : 0.0f; cosines[3 * i + 1] = has ? r.cos1 : 0.0f; cosines[3 * i + 2] = has ? r.cos2 : 0.0f;
        for (int a = 0; a < 4; a++) x3d[4 * i + a] = has ? r.x3D[a] : 0.0f;
    }
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}

}  // extern "C"

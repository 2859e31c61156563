// msl_plane.hip -- batched plane association and Manhattan-frame detection for gfx950.
//
// msl_plane_associate     PlaneMatcher::SearchMapByCoefficients (reference src/PlaneMatcher.cpp:31-106) with
//                         Frame::ComputePlaneWorldCoeff (src/Frame.cc:656-660)
// msl_manhattan_detect    Tracking::DetectManhattan (src/Tracking.cc:651-844) with Map::Get[Partial]ManhattanObservation (src/Map.cc:32-123)
//
// Frame batched, on the matcher handle's stream; three launches per pair of calls:
//   k_plane_dis     one wave per (map plane j, frame): the frame's <= 64 world coefficients pM in LDS, the plane's cloud read once per 16
//                   frame planes with per-lane minima of PointDistanceFromPlane in registers, then a DPP min-scan across the wave.  The minimum
//                   starts at 100 and a NaN distance never replaces it (`dis < res` is false), exactly as the reference loop; a minimum is
//                   order-independent, so the tree gives the loop's value.  Writes dis[f][j][k].
//   k_plane_assign  one wave per frame, lane k = frame plane k walking the map planes in order with the three running thresholds
//                   (a sequential walk: mcap <= 4096 and only the distance reads are memory traffic), then plane_match / plane_has / plane_w
//                   and nmatches.
//   k_manhattan     one workgroup per frame: every (i, j, k) triple and (i, j) pair is scored independently, the reference's "first candidate
//                   with the largest score > 0" is a 64-bit max of (score, ~order); lane 0 builds manhattanRcw from the winner.
#include "msl_match_handle.h"
#include "msl_match_math.h"

#include <algorithm>
#include <cmath>

using namespace msl;

namespace {

constexpr int MAX_PCAP = 64, MAX_MCAP = 4096, MAX_PTCAP = 1 << 22, MAX_FCAP = 65536, MAX_QCAP = 65536, MAX_KCAP = 4096;
constexpr int MF_NT = 256;
constexpr int KG = 16;                             // k_plane_dis: frame planes per pass over a cloud

struct AssocDev {
    int pcap, mcap, ptcap;
    msl_plane_params prm;
    const float *coef; const int32_t *nPlanes; const float *Tcw;
    const float *mpW; const uint8_t *mpFlags; const int32_t *mpOff; const float *mpPts; const int32_t *nMap;
    float *dis;                                     // [n][mcap][64] scratch
    int32_t *match, *nmatches; float *planeW; uint8_t *planeHas; float *pMOut;
};

struct MfDev {
    int pcap, mcap, fcap, qcap, kcap;
    msl_plane_params prm;
    const float *coef; const int32_t *npts, *nPlanes, *match; const uint8_t *mpFlags; const int32_t *nMap;
    const int32_t *fullTab, *nFull, *partTab, *nPart;
    const float *kfRwc, *kfCoef; const int32_t *kfNpts;
    float *Rcw; int32_t *found, *full, *choice;
};

__device__ __forceinline__ float minf_keep(float a, float b) { return b < a ? b : a; }   // NaN never wins (neither side holds one here)

// Wave-wide minimum of v (every lane gets it): a DPP inclusive min-scan, then lane 63 broadcast.  Lanes without a DPP source read 100,
// the loop's starting value, which every per-lane minimum already is below or equal to.
__device__ __forceinline__ float wave_min(float v) {
    const int fill = __float_as_int(100.0f);
    int x = __float_as_int(v);
    x = __float_as_int(minf_keep(__int_as_float(x), __int_as_float(__builtin_amdgcn_update_dpp(fill, x, 0x111, 0xF, 0xF, false))));
    x = __float_as_int(minf_keep(__int_as_float(x), __int_as_float(__builtin_amdgcn_update_dpp(fill, x, 0x112, 0xF, 0xF, false))));
    x = __float_as_int(minf_keep(__int_as_float(x), __int_as_float(__builtin_amdgcn_update_dpp(fill, x, 0x114, 0xF, 0xF, false))));
    x = __float_as_int(minf_keep(__int_as_float(x), __int_as_float(__builtin_amdgcn_update_dpp(fill, x, 0x118, 0xF, 0xF, false))));
    x = __float_as_int(minf_keep(__int_as_float(x), __int_as_float(__builtin_amdgcn_update_dpp(fill, x, 0x142, 0xA, 0xF, false))));
    x = __float_as_int(minf_keep(__int_as_float(x), __int_as_float(__builtin_amdgcn_update_dpp(fill, x, 0x143, 0xC, 0xF, false))));
    return __int_as_float(__builtin_amdgcn_readlane(x, 63));
}

__global__ __launch_bounds__(64) void k_plane_dis(AssocDev D) {
    const int f = blockIdx.x, j = blockIdx.y, lane = threadIdx.x;
    const int nMap = clampi(D.nMap[f], 0, D.mcap);
    if (j >= nMap) return;
    const int np = clampi(D.nPlanes[f], 0, D.pcap);
    __shared__ float pM[MAX_PCAP][4];
    if (lane < np) world_coef(D.Tcw + 12 * f, D.coef + ((size_t)f * D.pcap + lane) * 4, pM[lane]);
    __syncthreads();
    const int32_t *off = D.mpOff + (size_t)f * (D.mcap + 1);
    const int b = clampi(off[j], 0, D.ptcap), e = clampi(off[j + 1], b, D.ptcap);
    const float *pts = D.mpPts + (size_t)f * D.ptcap * 3;
    float mine = 100.0f;
    // Frame planes in groups of KG: KG running minima per lane stay in registers; the cloud is read once per group (np <= 64: at most
    // four times, the later passes from cache).
#pragma unroll 1
    for (int k0 = 0; k0 < np; k0 += KG) {
        float m[KG];
#pragma unroll
        for (int q = 0; q < KG; q++) m[q] = 100.0f;
        for (int p = b + lane; p < e; p += WAVE) {
            const float x = pts[3 * (size_t)p], y = pts[3 * (size_t)p + 1], z = pts[3 * (size_t)p + 2];
#pragma unroll
            for (int q = 0; q < KG; q++) {
                if (k0 + q < np) {   // src/PlaneMatcher.cpp:98-100: a float expression, left to right, then abs
                    const float *c = pM[k0 + q];
                    const float d = fabsf(c[0] * x + c[1] * y + c[2] * z + c[3]);
                    m[q] = minf_keep(m[q], d);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < KG; q++) {
            if (k0 + q < np) {
                const float v = wave_min(m[q]);
                if (lane == k0 + q) mine = v;
            }
        }
    }
    if (lane < np) D.dis[((size_t)f * D.mcap + j) * MAX_PCAP + lane] = mine;
}

__global__ __launch_bounds__(64) void k_plane_assign(AssocDev D) {
    const int f = blockIdx.x, k = threadIdx.x;
    const int np = clampi(D.nPlanes[f], 0, D.pcap), nMap = clampi(D.nMap[f], 0, D.mcap);
    bool found = false;
    if (k < np) {
        const size_t pk = (size_t)f * D.pcap + k;
        float pM[4];
        world_coef(D.Tcw + 12 * f, D.coef + pk * 4, pM);
        int32_t sel[3] = {D.match[3 * pk], D.match[3 * pk + 1], D.match[3 * pk + 2]};
        float ldTh = D.prm.d_th, lverTh = D.prm.ver_th, lparTh = D.prm.par_th;
        const float aTh = D.prm.a_th;
        for (int j = 0; j < nMap; j++) {
            const size_t mj = (size_t)f * D.mcap + j;
            if (!(D.mpFlags[mj] & 1)) continue;                              // isBad()
            const float *pW = D.mpW + 4 * mj;
            const float angle = pM[0] * pW[0] + pM[1] * pW[1] + pM[2] * pW[2];
            if (angle > aTh) {
                const float dis = D.dis[mj * MAX_PCAP + k];                  // a float value: the double compare is the float one
                if (dis < ldTh) { ldTh = dis; sel[0] = j; found = true; continue; }
            }
            if (angle < lverTh && angle > -lverTh) { lverTh = fabsf(angle); sel[2] = j; continue; }
            if (angle > lparTh || angle < -lparTh) { lparTh = fabsf(angle); sel[1] = j; }
        }
        uint8_t has = 0;
        for (int s = 0; s < 3; s++) {
            D.match[3 * pk + s] = sel[s];
            const bool ok = sel[s] >= 0 && sel[s] < nMap;
            has |= (uint8_t)((ok ? 1 : 0) << s);
            for (int c = 0; c < 4; c++)
                D.planeW[12 * pk + 4 * s + c] = ok ? D.mpW[4 * ((size_t)f * D.mcap + sel[s]) + c] : 0.0f;
        }
        D.planeHas[pk] = has;
        if (D.pMOut)
            for (int c = 0; c < 4; c++) D.pMOut[4 * pk + c] = pM[c];
    }
    const unsigned long long bal = __ballot(found);
    if (k == 0) D.nmatches[f] = __popcll(bal);
}

// ---- DetectManhattan ----

__device__ __forceinline__ float dot3_f32(const float *a, const float *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ bool mf_vertical(float a, float th) { return !(a > th || a < -th); }

// The map plane held by frame plane i (mvpMapPlanes[i]) when it is not NULL and not bad, else -1.
__device__ __forceinline__ int held(const MfDev &D, int f, int i, int nMap) {
    const int m = D.match[3 * ((size_t)f * D.pcap + i)];
    if (m < 0 || m >= nMap || !(D.mpFlags[(size_t)f * D.mcap + m] & 1)) return -1;
    return m;
}

__device__ __forceinline__ void sort3(int &a, int &b, int &c) {
    if (a > b) { int t = a; a = b; b = t; }
    if (b > c) { int t = b; b = c; c = t; }
    if (a > b) { int t = a; a = b; b = t; }
}

// Binary search of a table sorted ascending by its first w key ints (entries of `stride` ints); the entry index or -1.
__device__ int find_entry(const int32_t *tab, int n, int stride, int w, const int *key) {
    int lo = 0, hi = n - 1;
    while (lo <= hi) {
        const int mid = (lo + hi) >> 1;
        const int32_t *e = tab + (size_t)mid * stride;
        int c = 0;
        for (int q = 0; q < w && c == 0; q++) c = e[q] < key[q] ? -1 : (e[q] > key[q] ? 1 : 0);
        if (c == 0) return mid;
        if (c < 0) lo = mid + 1; else hi = mid - 1;
    }
    return -1;
}

// The keyframe plane index of map plane m in a table entry (the position of m among its sorted keys).
__device__ __forceinline__ int kf_index(const int32_t *e, int w, int m) {
    for (int q = 0; q < w; q++)
        if (e[q] == m) return e[w + 1 + q];
    return -1;
}

// The frame's planes as the candidate loop reads them, staged once per workgroup: the held map plane (held(), -1 = none), the coefficients
// and the point counts.
struct MfFrame {
    int held[MAX_PCAP];
    float coef[MAX_PCAP][4];
    int npts[MAX_PCAP];
};

// One candidate of the reference's loop order: c == n is the partial pair (i, j), c in (j, n) the triple (i, j, c).  Returns its score,
// or 0 when it is no candidate; *entry gets the table entry.
__device__ int score_of(const MfDev &D, const MfFrame &S, int f, int i, int j, int c, int np, int *entry) {
    const int m1 = S.held[i], m2 = S.held[j];
    if (m1 < 0 || m2 < 0) return 0;
    const float *c1 = S.coef[i], *c2 = S.coef[j];
    const float th = D.prm.mf_ver_th;
    if (!mf_vertical(dot3_f32(c1, c2), th)) return 0;                                    // angle12 (:675-681)
    const int kcap = D.kcap, pcap = D.pcap;
    if (c < np) {
        const int m3 = S.held[c];
        if (m3 < 0) return 0;
        const float *c3 = S.coef[c];
        if (!mf_vertical(dot3_f32(c1, c3), th) || !mf_vertical(dot3_f32(c2, c3), th)) return 0;   // (:691-701)
        int key[3] = {m1, m2, m3};
        sort3(key[0], key[1], key[2]);
        const int32_t *tab = D.fullTab + (size_t)f * D.fcap * 7;
        const int e = find_entry(tab, clampi(D.nFull[f], 0, D.fcap), 7, 3, key);
        if (e < 0) return 0;
        const int32_t *ent = tab + (size_t)e * 7;
        const int kf = ent[3], i1 = kf_index(ent, 3, m1), i2 = kf_index(ent, 3, m2), i3 = kf_index(ent, 3, m3);
        if (kf < 0 || kf >= kcap || i1 < 0 || i2 < 0 || i3 < 0 || i1 >= pcap || i2 >= pcap || i3 >= pcap) return 0;
        const int32_t *kn = D.kfNpts + ((size_t)f * kcap + kf) * pcap;
        *entry = e;
        return kn[i1] + kn[i2] + kn[i3] + S.npts[i] + S.npts[j] + S.npts[c];
    }
    int key[2] = {min(m1, m2), max(m1, m2)};
    const int32_t *tab = D.partTab + (size_t)f * D.qcap * 5;
    const int e = find_entry(tab, clampi(D.nPart[f], 0, D.qcap), 5, 2, key);
    if (e < 0) return 0;
    const int32_t *ent = tab + (size_t)e * 5;
    const int kf = ent[2], i1 = kf_index(ent, 2, m1), i2 = kf_index(ent, 2, m2);
    if (kf < 0 || kf >= kcap || i1 < 0 || i2 < 0 || i1 >= pcap || i2 >= pcap) return 0;
    const int32_t *kn = D.kfNpts + ((size_t)f * kcap + kf) * pcap;
    *entry = e;
    return kn[i1] + kn[i2] + S.npts[i] + S.npts[j];
}

// cv::gemm of two 3x3 CV_32F matrices (row-major; B transposed when tb): double accumulation, one rounding per element.
__device__ void gemm33(const float *A, const float *B, bool tb, float *C) {
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            double s = 0.0;
            for (int k = 0; k < 3; k++) s += (double)A[3 * r + k] * (double)(tb ? B[3 * c + k] : B[3 * k + c]);
            C[3 * r + c] = (float)s;
        }
}

// cv::determinant of a 3x3 CV_32F matrix (evaluated in double as OpenCV's det3 macro does).
__device__ double det3f(const float *m) {
    return m[0] * ((double)m[4] * m[8] - (double)m[5] * m[7]) - m[1] * ((double)m[3] * m[8] - (double)m[5] * m[6]) +
           m[2] * ((double)m[3] * m[7] - (double)m[4] * m[6]);
}

// The polar factor U * Vt of a 3x3 matrix, in double by Newton's iteration X <- (X + X^-T) / 2 (quadratic convergence for the
// well-conditioned Manhattan frames; stops when no entry moves by more than 1e-15, at most 60 steps), rounded to float.
__device__ void polar(const float *Mf, float *out) {
    double X[9];
    for (int q = 0; q < 9; q++) X[q] = Mf[q];
    for (int it = 0; it < 60; it++) {
        const double c00 = X[4] * X[8] - X[5] * X[7], c01 = X[5] * X[6] - X[3] * X[8], c02 = X[3] * X[7] - X[4] * X[6];
        const double c10 = X[2] * X[7] - X[1] * X[8], c11 = X[0] * X[8] - X[2] * X[6], c12 = X[1] * X[6] - X[0] * X[7];
        const double c20 = X[1] * X[5] - X[2] * X[4], c21 = X[2] * X[3] - X[0] * X[5], c22 = X[0] * X[4] - X[1] * X[3];
        const double det = X[0] * c00 + X[1] * c01 + X[2] * c02;
        if (!(det != 0.0)) break;
        const double cof[9] = {c00, c01, c02, c10, c11, c12, c20, c21, c22};      // X^-T = cofactor matrix / det
        double moved = 0.0;
        for (int q = 0; q < 9; q++) {
            const double nx = 0.5 * (X[q] + cof[q] / det);
            moved = fmax(moved, fabs(nx - X[q]));
            X[q] = nx;
        }
        if (moved <= 1e-15) break;
    }
    for (int q = 0; q < 9; q++) out[q] = (float)X[q];
}

__global__ __launch_bounds__(MF_NT) void k_manhattan(MfDev D) {
    const int f = blockIdx.x, t = threadIdx.x;
    const int np = clampi(D.nPlanes[f], 0, D.pcap), nMap = clampi(D.nMap[f], 0, D.mcap);
    __shared__ unsigned long long best;
    __shared__ MfFrame S;
    if (t == 0) best = 0ull;
    if (t < np) {
        S.held[t] = held(D, f, t, nMap);
        for (int q = 0; q < 4; q++) S.coef[t][q] = D.coef[((size_t)f * D.pcap + t) * 4 + q];
        S.npts[t] = D.npts[(size_t)f * D.pcap + t];
    }
    __syncthreads();
    // Candidate (i, j, c), c in (j, np]: the loop order is lexicographic in (i, j, c) with the pair (c = np) after the triples of (i, j).
    unsigned long long mine = 0ull;
    const int total = np * np * (np + 1);
    for (int q = t; q < total; q += MF_NT) {
        const int i = q / (np * (np + 1)), r = q - i * np * (np + 1), j = r / (np + 1), c = r - j * (np + 1);
        if (!(i < j && j < c)) continue;
        int e;
        const int s = score_of(D, S, f, i, j, c, np, &e);
        if (s <= 0) continue;
        const unsigned order = (unsigned)((i << 14) | (j << 7) | c);
        const unsigned long long key = ((unsigned long long)(unsigned)s << 32) | (0xFFFFFFFFu - order);
        mine = mine > key ? mine : key;
    }
    if (mine) atomicMax(&best, mine);
    __syncthreads();
    if (t != 0) return;
    const unsigned long long b = best;
    int32_t *ch = D.choice ? D.choice + 6 * (size_t)f : nullptr;
    if (!b) {
        D.found[f] = 0; D.full[f] = 0;
        if (ch) { ch[0] = -1; ch[1] = -1; ch[2] = -1; ch[3] = -1; ch[4] = 0; ch[5] = -1; }
        return;
    }
    const unsigned order = 0xFFFFFFFFu - (unsigned)(b & 0xFFFFFFFFull);
    const int i = order >> 14, j = (order >> 7) & 127, c = order & 127;
    const bool isFull = c < np;
    int e;
    const int score = score_of(D, S, f, i, j, c, np, &e);
    const int m1 = S.held[i], m2 = S.held[j];
    const int32_t *ent = isFull ? D.fullTab + ((size_t)f * D.fcap + e) * 7 : D.partTab + ((size_t)f * D.qcap + e) * 5;
    const int w = isFull ? 3 : 2, kf = ent[w];
    const float *kfc = D.kfCoef + ((size_t)f * D.kcap + kf) * D.pcap * 4;
    const float *pc1 = D.coef + ((size_t)f * D.pcap + i) * 4, *pc2 = D.coef + ((size_t)f * D.pcap + j) * 4;
    const float *pm1 = kfc + 4 * kf_index(ent, w, m1), *pm2 = kfc + 4 * kf_index(ent, w, m2);
    float c3[3], m3[3];
    if (isFull) {
        const float *pc3 = D.coef + ((size_t)f * D.pcap + c) * 4;
        const float *pm3 = kfc + 4 * kf_index(ent, w, S.held[c]);
        for (int q = 0; q < 3; q++) { c3[q] = pc3[q]; m3[q] = pm3[q]; }
    } else {                                                                      // cv::Mat::cross (:764-770), float
        c3[0] = pc1[1] * pc2[2] - pc1[2] * pc2[1]; c3[1] = pc1[2] * pc2[0] - pc1[0] * pc2[2]; c3[2] = pc1[0] * pc2[1] - pc1[1] * pc2[0];
        m3[0] = pm1[1] * pm2[2] - pm1[2] * pm2[1]; m3[1] = pm1[2] * pm2[0] - pm1[0] * pm2[2]; m3[2] = pm1[0] * pm2[1] - pm1[1] * pm2[0];
    }
    float MFc[9], MFm[9];
    for (int q = 0; q < 3; q++) {
        MFc[3 * q] = pc1[q]; MFc[3 * q + 1] = pc2[q]; MFc[3 * q + 2] = c3[q];
        MFm[3 * q] = pm1[q]; MFm[3 * q + 1] = pm2[q]; MFm[3 * q + 2] = m3[q];
    }
    if (!isFull && fabs(det3f(MFc) + 1) < 0.5)                                   // (:786-790), partial case only
        for (int q = 0; q < 3; q++) MFc[3 * q + 2] = -c3[q];
    if (!isFull && fabs(det3f(MFm) + 1) < 0.5)
        for (int q = 0; q < 3; q++) MFm[3 * q + 2] = -m3[q];
    float Pc[9], Pm[9], A[9], Rwc[9];
    polar(MFc, Pc);
    polar(MFm, Pm);
    gemm33(D.kfRwc + ((size_t)f * D.kcap + kf) * 9, Pm, false, A);             // (GetPoseInverse()(0:3, 0:3) * MFm) * MFc^T
    gemm33(A, Pc, true, Rwc);
    float *R = D.Rcw + 9 * (size_t)f;
    for (int r = 0; r < 3; r++)
        for (int q = 0; q < 3; q++) R[3 * r + q] = Rwc[3 * q + r];               // manhattanRcw = Rwc^T
    D.found[f] = 1; D.full[f] = isFull ? 1 : 0;
    if (ch) { ch[0] = i; ch[1] = j; ch[2] = isFull ? c : -1; ch[3] = e; ch[4] = score; ch[5] = kf; }
}

// Host tables must be sorted ascending by their keys, each key ascending within the entry.
bool table_sorted(const int32_t *tab, int n, int stride, int w) {
    for (int e = 0; e < n; e++) {
        const int32_t *x = tab + (size_t)e * stride;
        for (int q = 1; q < w; q++)
            if (x[q - 1] > x[q]) return false;
        if (e > 0 && !std::lexicographical_compare(x - stride, x - stride + w, x, x + w)) return false;
    }
    return true;
}

int run_associate(msl_match *h, int n_frames, int pcap, int mcap, int ptcap, const msl_plane_params *prm, const float *plane_coef,
                  const int32_t *n_planes, const float *Tcw, const float *mp_w, const uint8_t *mp_flags, const int32_t *mp_pt_off,
                  const float *mp_pts, const int32_t *n_map, msl_mem mem, int32_t *plane_match, int32_t *nmatches, float *plane_w,
                  uint8_t *plane_has, float *pM_out, msl_mem out_mem) {
    if (!h || n_frames < 1 || pcap < 1 || pcap > MAX_PCAP || mcap < 1 || mcap > MAX_MCAP || ptcap < 1 || ptcap > MAX_PTCAP || !prm ||
        !plane_coef || !n_planes || !Tcw || !mp_w || !mp_flags || !mp_pt_off || !mp_pts || !n_map || !plane_match || !nmatches ||
        !plane_w || !plane_has) {
        set_error("msl_plane_associate: invalid argument (1 <= pcap <= %d, mcap <= %d, ptcap <= %d)", MAX_PCAP, MAX_MCAP, MAX_PTCAP);
        return MSL_ERR_INVALID;
    }
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    hipStream_t st = h->stream;
    const size_t F = (size_t)n_frames, p = F * pcap, m = F * mcap;
    AssocDev D{};
    D.pcap = pcap; D.mcap = mcap; D.ptcap = ptcap; D.prm = *prm;
    Stage S(h, mem, out_mem);
    D.coef = S.in(plane_coef, 4 * p); D.nPlanes = S.in(n_planes, F); D.Tcw = S.in(Tcw, 12 * F); D.mpW = S.in(mp_w, 4 * m);
    D.mpFlags = S.in(mp_flags, m); D.mpOff = S.in(mp_pt_off, m + F); D.mpPts = S.in(mp_pts, 3 * F * ptcap); D.nMap = S.in(n_map, F);
    D.match = S.inout(plane_match, 3 * p);                                     // the entries a search does not replace stay
    D.nmatches = S.out(nmatches, F); D.planeW = S.out(plane_w, 12 * p); D.planeHas = S.out(plane_has, p); D.pMOut = S.out(pM_out, 4 * p);
    MSL_HIP_TRY(S.error());
    MSL_HIP_TRY(h->planeDis.grow(sizeof(float) * m * MAX_PCAP, st));
    D.dis = (float *)h->planeDis.p;
    hipLaunchKernelGGL(k_plane_dis, dim3((unsigned)n_frames, (unsigned)mcap), dim3(64), 0, st, D);
    MSL_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_plane_assign, dim3((unsigned)n_frames), dim3(64), 0, st, D);
    MSL_HIP_TRY(hipGetLastError());
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}

int run_manhattan(msl_match *h, int n_frames, int pcap, int mcap, int fcap, int qcap, int kcap, const msl_plane_params *prm,
                  const float *plane_coef, const int32_t *plane_npts, const int32_t *n_planes, const int32_t *plane_match,
                  const uint8_t *mp_flags, const int32_t *n_map, const int32_t *full_tab, const int32_t *n_full, const int32_t *part_tab,
                  const int32_t *n_part, const float *kf_Rwc, const float *kf_coef, const int32_t *kf_npts, msl_mem mem, int32_t *found,
                  int32_t *full, float *Rcw, int32_t *choice, msl_mem out_mem) {
    if (!h || n_frames < 1 || pcap < 1 || pcap > MAX_PCAP || mcap < 1 || mcap > MAX_MCAP || fcap < 1 || fcap > MAX_FCAP || qcap < 1 ||
        qcap > MAX_QCAP || kcap < 1 || kcap > MAX_KCAP || !prm || !plane_coef || !plane_npts || !n_planes || !plane_match || !mp_flags ||
        !n_map || !full_tab || !n_full || !part_tab || !n_part || !kf_Rwc || !kf_coef || !kf_npts || !found || !full || !Rcw) {
        set_error("msl_manhattan_detect: invalid argument (1 <= pcap <= %d, mcap <= %d, fcap <= %d, qcap <= %d, kcap <= %d)", MAX_PCAP,
                  MAX_MCAP, MAX_FCAP, MAX_QCAP, MAX_KCAP);
        return MSL_ERR_INVALID;
    }
    if (mem == MSL_MEM_HOST)
        for (int f = 0; f < n_frames; f++) {
            const int nf = std::min(std::max(n_full[f], 0), fcap), nq = std::min(std::max(n_part[f], 0), qcap);
            if (!table_sorted(full_tab + (size_t)f * fcap * 7, nf, 7, 3) || !table_sorted(part_tab + (size_t)f * qcap * 5, nq, 5, 2)) {
                set_error("msl_manhattan_detect: the Manhattan tables of frame %d are not sorted by their keys", f);
                return MSL_ERR_INVALID;
            }
        }
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    hipStream_t st = h->stream;
    const size_t F = (size_t)n_frames, p = F * pcap, m = F * mcap, k = F * kcap;
    MfDev D{};
    D.pcap = pcap; D.mcap = mcap; D.fcap = fcap; D.qcap = qcap; D.kcap = kcap; D.prm = *prm;
    Stage S(h, mem, out_mem);
    D.coef = S.in(plane_coef, 4 * p); D.npts = S.in(plane_npts, p); D.nPlanes = S.in(n_planes, F); D.match = S.in(plane_match, 3 * p);
    D.mpFlags = S.in(mp_flags, m); D.nMap = S.in(n_map, F); D.fullTab = S.in(full_tab, 7 * F * fcap); D.nFull = S.in(n_full, F);
    D.partTab = S.in(part_tab, 5 * F * qcap); D.nPart = S.in(n_part, F); D.kfRwc = S.in(kf_Rwc, 9 * k); D.kfCoef = S.in(kf_coef, 4 * k * pcap);
    D.kfNpts = S.in(kf_npts, k * pcap);
    D.Rcw = S.inout(Rcw, 9 * F);                                               // written only where found
    D.found = S.out(found, F); D.full = S.out(full, F); D.choice = S.out(choice, 6 * F);
    MSL_HIP_TRY(S.error());
    hipLaunchKernelGGL(k_manhattan, dim3((unsigned)n_frames), dim3(MF_NT), 0, st, D);
    MSL_HIP_TRY(hipGetLastError());
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}

}  // namespace

extern "C" {

int msl_plane_associate(msl_match *h, int n_frames, int pcap, int mcap, int ptcap, const msl_plane_params *params, const float *plane_coef,
                        const int32_t *n_planes, const float *Tcw, const float *mp_w, const uint8_t *mp_flags, const int32_t *mp_pt_off,
                        const float *mp_pts, const int32_t *n_map, msl_mem mem, int32_t *plane_match, int32_t *nmatches, float *plane_w,
                        uint8_t *plane_has, float *pM_out, msl_mem out_mem) noexcept {
    try {
    return run_associate(h, n_frames, pcap, mcap, ptcap, params, plane_coef, n_planes, Tcw, mp_w, mp_flags, mp_pt_off, mp_pts, n_map, mem, plane_match,
                         nmatches, plane_w, plane_has, pM_out, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_plane_associate_batch(int device, int n_frames, int pcap, int mcap, int ptcap, const msl_plane_params *params,
                              const float *plane_coef, const int32_t *n_planes, const float *Tcw, const float *mp_w, const uint8_t *mp_flags,
                              const int32_t *mp_pt_off, const float *mp_pts, const int32_t *n_map, msl_mem mem, int32_t *plane_match,
                              int32_t *nmatches, float *plane_w, uint8_t *plane_has, float *pM_out, msl_mem out_mem) noexcept {
    // plane_match is an input too: device-memory outputs are read as well
    try {
    return abi_call_default(run_associate, device, mem == MSL_MEM_DEVICE || out_mem == MSL_MEM_DEVICE, n_frames, pcap, mcap, ptcap, params, plane_coef,
                            n_planes, Tcw, mp_w, mp_flags, mp_pt_off, mp_pts, n_map, mem, plane_match, nmatches, plane_w, plane_has, pM_out, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_manhattan_detect(msl_match *h, int n_frames, int pcap, int mcap, int fcap, int qcap, int kcap, const msl_plane_params *params,
                         const float *plane_coef, const int32_t *plane_npts, const int32_t *n_planes, const int32_t *plane_match,
                         const uint8_t *mp_flags, const int32_t *n_map, const int32_t *full_tab, const int32_t *n_full,
                         const int32_t *part_tab, const int32_t *n_part, const float *kf_Rwc, const float *kf_coef, const int32_t *kf_npts,
                         msl_mem mem, int32_t *found, int32_t *full, float *Rcw, int32_t *choice, msl_mem out_mem) noexcept {
    try {
    return run_manhattan(h, n_frames, pcap, mcap, fcap, qcap, kcap, params, plane_coef, plane_npts, n_planes, plane_match, mp_flags, n_map, full_tab, n_full,
                         part_tab, n_part, kf_Rwc, kf_coef, kf_npts, mem, found, full, Rcw, choice, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_manhattan_detect_batch(int device, int n_frames, int pcap, int mcap, int fcap, int qcap, int kcap, const msl_plane_params *params,
                               const float *plane_coef, const int32_t *plane_npts, const int32_t *n_planes, const int32_t *plane_match,
                               const uint8_t *mp_flags, const int32_t *n_map, const int32_t *full_tab, const int32_t *n_full,
                               const int32_t *part_tab, const int32_t *n_part, const float *kf_Rwc, const float *kf_coef,
                               const int32_t *kf_npts, msl_mem mem, int32_t *found, int32_t *full, float *Rcw, int32_t *choice,
                               msl_mem out_mem) noexcept {
    // Rcw is in/out: device-memory outputs are read as well
    try {
    return abi_call_default(run_manhattan, device, mem == MSL_MEM_DEVICE || out_mem == MSL_MEM_DEVICE, n_frames, pcap, mcap, fcap, qcap, kcap, params,
                            plane_coef, plane_npts, n_planes, plane_match, mp_flags, n_map, full_tab, n_full, part_tab, n_part, kf_Rwc, kf_coef, kf_npts, mem,
                            found, full, Rcw, choice, out_mem);
    } MSL_ABI_CATCH_INT
}

}  // extern "C"

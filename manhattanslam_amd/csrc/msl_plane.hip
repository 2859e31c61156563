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
#include "msl_index_check.h"
#include "msl_match_handle.h"
#include "msl_match_math.h"
#include "msl_plane_tables.h"

#include <climits>
#include <cmath>

using namespace msl;

namespace {

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

// The entry of a table (n entries of key width w, sorted ascending by their keys) that has `key`, or -1.  k_manhattan keeps this closed
// interval with its early return: as lower_bound_key plus its `found` (msl_plane_tables.h) the kernel comes out 44 instructions longer,
// and nothing here measures its rate.  The two agree on every table without duplicate keys.
__device__ int find_entry(const int32_t *tab, int n, int w, const int *key) {
    const int stride = mf::stride(w);
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

// The frame's planes as the candidate loop reads them, staged once per workgroup: the held map plane (held_row(), -1 = none), the coefficients
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
        constexpr int W = mf::FULL, ST = mf::stride(W);
        const int32_t *tab = D.fullTab + (size_t)f * D.fcap * ST;
        const int e = find_entry(tab, clampi(D.nFull[f], 0, D.fcap), W, key);
        if (e < 0) return 0;
        const int32_t *ent = tab + (size_t)e * ST;
        const int kf = ent[mf::kf_at(W)], i1 = kf_index(ent, W, m1), i2 = kf_index(ent, W, m2), i3 = kf_index(ent, W, m3);
        if (kf < 0 || kf >= kcap || i1 < 0 || i2 < 0 || i3 < 0 || i1 >= pcap || i2 >= pcap || i3 >= pcap) return 0;
        const int32_t *kn = D.kfNpts + ((size_t)f * kcap + kf) * pcap;
        *entry = e;
        return kn[i1] + kn[i2] + kn[i3] + S.npts[i] + S.npts[j] + S.npts[c];
    }
    int key[2] = {min(m1, m2), max(m1, m2)};
    constexpr int W = mf::PART, ST = mf::stride(W);
    const int32_t *tab = D.partTab + (size_t)f * D.qcap * ST;
    const int e = find_entry(tab, clampi(D.nPart[f], 0, D.qcap), W, key);
    if (e < 0) return 0;
    const int32_t *ent = tab + (size_t)e * ST;
    const int kf = ent[mf::kf_at(W)], i1 = kf_index(ent, W, m1), i2 = kf_index(ent, W, m2);
    if (kf < 0 || kf >= kcap || i1 < 0 || i2 < 0 || i1 >= pcap || i2 >= pcap) return 0;
    const int32_t *kn = D.kfNpts + ((size_t)f * kcap + kf) * pcap;
    *entry = e;
    return kn[i1] + kn[i2] + S.npts[i] + S.npts[j];
}

// cv::gemm of two 3x3 CV_32F matrices (row-major; B transposed when tb): double accumulation, one rounding per element.  Not
// msl_match_math.h's gemm33<SA, SB>: that one rounds s * alpha + 0.0, which turns a sum of -0 into +0 and changes k_manhattan's text.
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
        S.held[t] = held_row(D.match[3 * ((size_t)f * D.pcap + t)], D.mpFlags + (size_t)f * D.mcap, nMap);
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
    const int32_t *ent = isFull ? D.fullTab + ((size_t)f * D.fcap + e) * mf::stride(mf::FULL) : D.partTab + ((size_t)f * D.qcap + e) * mf::stride(mf::PART);
    const int w = isFull ? mf::FULL : mf::PART, kf = ent[mf::kf_at(w)];
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

const char *const WHO_PA = "msl_plane_associate", *const WHO_MD = "msl_manhattan_detect";

int check_associate(int n_frames, int pcap, int mcap, int ptcap, const msl_plane_params *params, const float *plane_coef, const int32_t *n_planes,
                    const float *Tcw, const float *mp_w, const uint8_t *mp_flags, const int32_t *mp_pt_off, const float *mp_pts,
                    const int32_t *n_map, msl_mem, int32_t *plane_match, int32_t *nmatches, float *plane_w, uint8_t *plane_has, float *,
                    msl_mem) {
    const char *who = WHO_PA;
    if (!none_null(who, {MSL_NAMED(params), MSL_NAMED(plane_coef), MSL_NAMED(n_planes), MSL_NAMED(Tcw), MSL_NAMED(mp_w), MSL_NAMED(mp_flags),
                         MSL_NAMED(mp_pt_off), MSL_NAMED(mp_pts), MSL_NAMED(n_map), MSL_NAMED(plane_match), MSL_NAMED(nmatches),
                         MSL_NAMED(plane_w), MSL_NAMED(plane_has)})) return MSL_ERR_INVALID;
    if (!in_range(who, "n_frames", n_frames, 1, INT_MAX) || !in_range(who, "pcap", pcap, 1, MAX_PCAP) ||
        !in_range(who, "mcap", mcap, 1, MAX_PLANE_MCAP) || !in_range(who, "ptcap", ptcap, 1, MAX_PLANE_PTCAP)) return MSL_ERR_INVALID;
    return MSL_OK;
}

int launch_associate(msl_match *h, int n_frames, int pcap, int mcap, int ptcap, const msl_plane_params *prm, const float *plane_coef,
                     const int32_t *n_planes, const float *Tcw, const float *mp_w, const uint8_t *mp_flags, const int32_t *mp_pt_off,
                     const float *mp_pts, const int32_t *n_map, msl_mem mem, int32_t *plane_match, int32_t *nmatches, float *plane_w,
                     uint8_t *plane_has, float *pM_out, msl_mem out_mem) {
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

// Host tables must be sorted ascending by their keys, each key ascending within the entry; the counts are clamped, as the kernel clamps them.
int check_manhattan(int n_frames, int pcap, int mcap, int fcap, int qcap, int kcap, const msl_plane_params *params, const float *plane_coef,
                    const int32_t *plane_npts, const int32_t *n_planes, const int32_t *plane_match, const uint8_t *mp_flags,
                    const int32_t *n_map, const int32_t *full_tab, const int32_t *n_full, const int32_t *part_tab, const int32_t *n_part,
                    const float *kf_Rwc, const float *kf_coef, const int32_t *kf_npts, msl_mem mem, int32_t *found, int32_t *full, float *Rcw,
                    int32_t *, msl_mem) {
    const char *who = WHO_MD;
    if (!none_null(who, {MSL_NAMED(params), MSL_NAMED(plane_coef), MSL_NAMED(plane_npts), MSL_NAMED(n_planes), MSL_NAMED(plane_match),
                         MSL_NAMED(mp_flags), MSL_NAMED(n_map), MSL_NAMED(full_tab), MSL_NAMED(n_full), MSL_NAMED(part_tab), MSL_NAMED(n_part),
                         MSL_NAMED(kf_Rwc), MSL_NAMED(kf_coef), MSL_NAMED(kf_npts), MSL_NAMED(found), MSL_NAMED(full), MSL_NAMED(Rcw)}))
        return MSL_ERR_INVALID;
    if (!in_range(who, "n_frames", n_frames, 1, INT_MAX) || !in_range(who, "pcap", pcap, 1, MAX_PCAP) ||
        !in_range(who, "mcap", mcap, 1, MAX_PLANE_MCAP) || !in_range(who, "fcap", fcap, 1, MAX_FCAP) ||
        !in_range(who, "qcap", qcap, 1, MAX_QCAP) || !in_range(who, "kcap", kcap, 1, MAX_PLANE_KCAP)) return MSL_ERR_INVALID;
    char why[256];
    if (mem == MSL_MEM_HOST &&
        (!check::tables_sorted_ok("full_tab", n_frames, fcap, mf::stride(mf::FULL), mf::FULL, full_tab, n_full, why, sizeof(why)) ||
         !check::tables_sorted_ok("part_tab", n_frames, qcap, mf::stride(mf::PART), mf::PART, part_tab, n_part, why, sizeof(why))))
        return refuse(who, why);
    return MSL_OK;
}

int launch_manhattan(msl_match *h, int n_frames, int pcap, int mcap, int fcap, int qcap, int kcap, const msl_plane_params *prm,
                     const float *plane_coef, const int32_t *plane_npts, const int32_t *n_planes, const int32_t *plane_match,
                     const uint8_t *mp_flags, const int32_t *n_map, const int32_t *full_tab, const int32_t *n_full, const int32_t *part_tab,
                     const int32_t *n_part, const float *kf_Rwc, const float *kf_coef, const int32_t *kf_npts, msl_mem mem, int32_t *found,
                     int32_t *full, float *Rcw, int32_t *choice, msl_mem out_mem) {
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    hipStream_t st = h->stream;
    const size_t F = (size_t)n_frames, p = F * pcap, m = F * mcap, k = F * kcap;
    MfDev D{};
    D.pcap = pcap; D.mcap = mcap; D.fcap = fcap; D.qcap = qcap; D.kcap = kcap; D.prm = *prm;
    Stage S(h, mem, out_mem);
    D.coef = S.in(plane_coef, 4 * p); D.npts = S.in(plane_npts, p); D.nPlanes = S.in(n_planes, F); D.match = S.in(plane_match, 3 * p);
    D.mpFlags = S.in(mp_flags, m); D.nMap = S.in(n_map, F);
    D.fullTab = S.in(full_tab, mf::stride(mf::FULL) * F * fcap); D.nFull = S.in(n_full, F);
    D.partTab = S.in(part_tab, mf::stride(mf::PART) * F * qcap); D.nPart = S.in(n_part, F);
    D.kfRwc = S.in(kf_Rwc, 9 * k); D.kfCoef = S.in(kf_coef, 4 * k * pcap); D.kfNpts = S.in(kf_npts, k * pcap);
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
    return handle_form(WHO_PA, check_associate, launch_associate, h, n_frames, pcap, mcap, ptcap, params, plane_coef, n_planes, Tcw, mp_w, mp_flags,
                       mp_pt_off, mp_pts, n_map, mem, plane_match, nmatches, plane_w, plane_has, pM_out, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_plane_associate_batch(int device, int n_frames, int pcap, int mcap, int ptcap, const msl_plane_params *params,
                              const float *plane_coef, const int32_t *n_planes, const float *Tcw, const float *mp_w, const uint8_t *mp_flags,
                              const int32_t *mp_pt_off, const float *mp_pts, const int32_t *n_map, msl_mem mem, int32_t *plane_match,
                              int32_t *nmatches, float *plane_w, uint8_t *plane_has, float *pM_out, msl_mem out_mem) noexcept {
    // plane_match is an input too: device-memory outputs are read as well
    try {
    return batch_form(check_associate, launch_associate, device, mem == MSL_MEM_DEVICE || out_mem == MSL_MEM_DEVICE, n_frames, pcap, mcap, ptcap,
                      params, plane_coef, n_planes, Tcw, mp_w, mp_flags, mp_pt_off, mp_pts, n_map, mem, plane_match, nmatches, plane_w, plane_has,
                      pM_out, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_manhattan_detect(msl_match *h, int n_frames, int pcap, int mcap, int fcap, int qcap, int kcap, const msl_plane_params *params,
                         const float *plane_coef, const int32_t *plane_npts, const int32_t *n_planes, const int32_t *plane_match,
                         const uint8_t *mp_flags, const int32_t *n_map, const int32_t *full_tab, const int32_t *n_full,
                         const int32_t *part_tab, const int32_t *n_part, const float *kf_Rwc, const float *kf_coef, const int32_t *kf_npts,
                         msl_mem mem, int32_t *found, int32_t *full, float *Rcw, int32_t *choice, msl_mem out_mem) noexcept {
    try {
    return handle_form(WHO_MD, check_manhattan, launch_manhattan, h, n_frames, pcap, mcap, fcap, qcap, kcap, params, plane_coef, plane_npts, n_planes,
                       plane_match, mp_flags, n_map, full_tab, n_full, part_tab, n_part, kf_Rwc, kf_coef, kf_npts, mem, found, full, Rcw, choice,
                       out_mem);
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
    return batch_form(check_manhattan, launch_manhattan, device, mem == MSL_MEM_DEVICE || out_mem == MSL_MEM_DEVICE, n_frames, pcap, mcap, fcap, qcap,
                      kcap, params, plane_coef, plane_npts, n_planes, plane_match, mp_flags, n_map, full_tab, n_full, part_tab, n_part, kf_Rwc,
                      kf_coef, kf_npts, mem, found, full, Rcw, choice, out_mem);
    } MSL_ABI_CATCH_INT
}

}  // extern "C"

// msl_match.hip -- batched Hamming matching by projection for gfx950.
//
// Replaces ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th) (reference src/ORBmatcher.cc:547-678)
// with Frame::GetFeaturesInArea (src/Frame.cc:332-381), ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:835-849) and the
// rotation-consistency histogram (ComputeThreeMaxima, :799-830), for many independent frame pairs per call.
//
// MI355X-first structure (frame-batched: blockIdx.y = pair), three launches per call:
//   k_match_grid        one workgroup per pair: the 64 x 48 feature grid of the current frame as a cell-sorted item list
//                       (counting sort in LDS; ascending cell id, ascending keypoint index inside a cell = mGrid insertion order)
//                       + the forward / backward search mode of the pair (:560-571);
//   k_match_candidates  one wave per last-frame point: projection (:577-593), window cells spread over the lanes, level /
//                       distance / mvuRight filters (:596-628, Frame.cc:353-376), 256-bit Hamming distance by v_bcnt on 8 dwords;
//                       candidates are stored as (distance << 16 | position in the item list).  The window is walked in
//                       ascending cell id and a cell's items in insertion order, so "first candidate wins ties" (:635) is the
//                       minimum of that packed key and the candidates need not be stored in order;
//   k_match_assign      one workgroup per pair: the reference's greedy, order dependent assignment (:621-623: a candidate held by
//                       a point with Observations() > 0 is skipped; :638: later points overwrite earlier ones) as the min-fixpoint
//                       of msl_assign.h (greedy_assign: round loop, holder = last picker, match count; the argument is there).
//                       Then rotation histogram, three maxima, NULLing (:657-674; rotation_cull in msl_match_math.h).
//
// Integer / byte work, L2-resident gathers; no MFMA.  The float expressions keep the reference's order; the 3x3 cv::Mat products
// follow cv::gemm's float kernel (double accumulation, one rounding) -- pinned in DESIGN.md section 3; gemm3, the search mode, the popcount
// and predict_scale live in msl_match_math.h, shared with the line matcher (msl_line_match.hip).  This file also defines msl::Stage
// (msl_match_handle.h), the staging of host-memory arguments every entry point on the handle uses.
#include "msl_assign.h"
#include "msl_match_handle.h"
#include "msl_match_math.h"
#include "msl_match_window.h"

#include <climits>
#include <mutex>
#include <new>

using namespace msl;

msl_match *msl::g_default[16];
std::mutex msl::g_default_mutex;

namespace {

constexpr int TH_HIGH = 100, HISTO_LENGTH = 30;     // src/ORBmatcher.cc:33-35
static_assert(HISTO_LENGTH == ROT_HISTO_LENGTH, "rot_bin / three_maxima (msl_match_math.h) use the same histogram");

// ---- k_match_candidates: one wave per last-frame point ----------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_match_candidates(MatchDev P) {
    __shared__ unsigned s_cnt[4];
    const int pair = blockIdx.y, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + wv;
    if (q >= min(P.nLast[pair], P.cap)) return;
    const size_t qi = (size_t)pair * P.cap + q;
    if (lane == 0) s_cnt[wv] = 0;
    __builtin_amdgcn_wave_barrier();
    Query Q;
    const bool live = (P.lastFlags[qi] & 1) && project_query(P, pair, q, P.mode[pair], Q);
    if (!live) {
        if (lane == 0) P.candCnt[qi] = 0;
        return;
    }
    wave_candidates(P, pair, Q, P.lastDesc + qi * 32, DIST_ANY, P.cand + qi * CMAX, &s_cnt[wv], lane);
    if (lane == 0) P.candCnt[qi] = s_cnt[wv];
}

// ---- k_match_assign: one workgroup per pair ------------------------------------------------------------------------------------
constexpr int ASSIGN_NT = 1024;

__global__ __launch_bounds__(ASSIGN_NT) void k_match_assign(MatchDev P) {
    extern __shared__ int s_dyn[];          // t[cap], then the holder | rotation bin[cap] | pick[cap] short (inside the third int[cap])
    __shared__ int s_hist[HISTO_LENGTH], s_keep[3], s_nm;
    const int pair = blockIdx.x;
    const int nLast = min(P.nLast[pair], P.cap), nCur = min(P.nCur[pair], P.cap), mode = P.mode[pair];
    int *s_t = s_dyn, *s_bin = s_dyn + P.cap;
    short *s_pick = reinterpret_cast<short *>(s_dyn + 2 * P.cap);   // current-frame keypoint picked by each point, -1 = none
    const unsigned short *items = P.items + (size_t)pair * P.cap;
    const size_t base = (size_t)pair * P.cap;
    if (threadIdx.x < HISTO_LENGTH) s_hist[threadIdx.x] = 0;

    // point q's choice given the current t: the minimum of (dist << 16 | item position) over the candidates it does not skip, bestDist <= TH_HIGH (:637)
    auto pick_of = [&](int q) -> int {
        unsigned best = KEY_NONE;
        unskipped_candidates(P, pair, base + q, q, P.lastDesc + (base + q) * 32, DIST_ANY, s_t,
                             [&](Query &Q) { return project_query(P, pair, q, mode, Q); }, [&](unsigned key) { best = min(best, key); });
        return (best != KEY_NONE && (int)(best >> 16) <= TH_HIGH) ? (int)items[best & 0xFFFFu] : -1;
    };
    // the greedy hand-out of :621-623 / :638 (msl_assign.h); nothing is held on entry
    greedy_assign<ASSIGN_NT>(nLast, nCur, s_t, s_pick, &s_nm, pick_of, [&](int q) { return (P.lastFlags[base + q] & 2) != 0; },
                             [](int) { return T_FREE; });
    if (P.prm.check_orientation) {          // rotation histogram, three maxima, NULLing (:643-649, :657-674)
        for (int q = threadIdx.x; q < nLast; q += ASSIGN_NT)
            s_bin[q] = s_pick[q] >= 0 ? rot_bin(P.lastAngle[base + q] - P.curKps[base + s_pick[q]].angle) : -1;
        rotation_cull<ASSIGN_NT>(nLast, s_hist, s_keep, [&](int q) { return s_bin[q]; }, [&](int q) {
            s_t[s_pick[q]] = -1;
            atomicSub(&s_nm, 1);
        });
    }
    for (int i = threadIdx.x; i < P.cap; i += ASSIGN_NT) P.matchOut[base + i] = i < nCur ? s_t[i] : -1;
    if (threadIdx.x == 0) P.nmatches[pair] = s_nm;
}

// ==== Matching the local map: Tracking::SearchLocalPoints (src/Tracking.cc:1654-1695) ======================================================
// Frame-batched (blockIdx.y / blockIdx.x = frame), four launches per call, the first of them k_match_grid above (no last frame: mode == nullptr):
//   k_local_frustum     one lane per local map point: Frame::isInFrustum (src/Frame.cc:204-259) + MapPoint::PredictScale (src/MapPoint.cc:350-364)
//                       -> mbTrackInView and the track record (mTrackProjX / Y / XR, mnTrackScaleLevel, mTrackViewCos);
//   k_local_candidates  one wave per point in view: window of RadiusByViewingCos (src/ORBmatcher.cc:119-124) * th * mvScaleFactors[L], levels
//                       [L-1, L] (GetFeaturesInArea's bCheckLevels rule), the mvuRight test on mTrackProjXR (:84-88), Hamming distance; stored as
//                       (dist << 16 | item position) by wave_candidates exactly as for the last-frame search;
//   k_local_assign      one workgroup per frame: SearchByProjection's greedy hand-out (:51-112) as the min-fixpoint of msl_assign.h (point j =
//                       position in mvpLocalMapPoints), then nToMatch.
// Best / second best of point j.  Positions in the item list ascend in the reference's walk order (cell ix * 48 + iy, mGrid insertion order
// inside a cell), and the reference's update rule (:94-103: strict < for both) leaves (bestIdx, bestLevel) = the smallest (dist, position)
// key and (bestDist2, bestLevel2) = the second smallest among the candidates it did not skip, ignoring distance 256 (never < the initial
// 256).  So pick(j) is a function of the set of keypoints point j skips, as the hand-out requires.
// LDS of k_local_assign: t[cap] int + pick[mcap] short = 4 cap + 2 mcap bytes, 96 KB at the limits (cap 8192, mcap 32768): inside the 160 KB
// of a CDNA4 CU, and no more than k_match_assign asks for at its own limit, so the scratch never spills to global memory.
constexpr int LOCAL_NT = 1024;

struct LocalDev {
    MatchDev m;                                     // current frame, grid scratch, candidates (per local point), params (m.prm = base), matchOut, nmatches
    int mcap;
    float logScale, viewCosLimit, nnRatio;
    const uint8_t *curFlags;
    const float *mpXyz, *mpNormal, *mpDist; const uint8_t *mpDesc, *mpFlags; const int32_t *nLocal;
    uint8_t *inView; msl_local_track *track;        // [n][mcap] scratch read by the later launches
    uint8_t *inViewOut; msl_local_track *trackOut;  // the caller's device arrays (or nullptr)
    int32_t *nToMatch;
};

// ---- k_local_frustum: one lane per local map point --------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_local_frustum(LocalDev L) {
    const int f = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= min(L.nLocal[f], L.mcap)) return;
    const MatchDev &P = L.m;
    const size_t jj = (size_t)f * L.mcap + j;
    msl_local_track t{0.0f, 0.0f, 0.0f, 0, 0.0f};
    uint8_t in = 0;
    if (L.mpFlags[jj] & 1) {   // SearchLocalPoints skips bad points and points already seen in this frame (:1672-1675)
        const float *Tc = P.TcwCur + (size_t)f * 12;
        const float tcw[3] = {Tc[3], Tc[7], Tc[11]};
        const float Pw[3] = {L.mpXyz[3 * jj], L.mpXyz[3 * jj + 1], L.mpXyz[3 * jj + 2]};
        float Pc[3];
        gemm3(Tc, false, 1.0, Pw, tcw, Pc);                               // Pc = mRcw * P + mtcw (:211)
        const float PcX = Pc[0], PcY = Pc[1], PcZ = Pc[2];
        if (!(PcZ < 0.0f)) {                                              // :217-218
            const float invz = 1.0f / PcZ;
            const float u = P.prm.fx * PcX * invz + P.prm.cx;              // :221-223, left to right, no contraction
            const float v = P.prm.fy * PcY * invz + P.prm.cy;
            if (!(u < P.prm.minX || u > P.prm.maxX) && !(v < P.prm.minY || v > P.prm.maxY)) {   // :225-228 (a NaN passes, as there)
                float Ow[3];
                gemm3(Tc, true, -1.0, tcw, nullptr, Ow);                   // mOw = -mRcw.t() * mtcw (Frame::UpdatePoseMatrices)
                const float PO[3] = {Pw[0] - Ow[0], Pw[1] - Ow[1], Pw[2] - Ow[2]};
                double ss = 0.0;
                for (int k = 0; k < 3; k++) ss += (double)PO[k] * (double)PO[k];
                const float dist = (float)sqrt(ss);                         // cv::norm on CV_32F (:234)
                const float dmin = L.mpDist[2 * jj], dmax = L.mpDist[2 * jj + 1];
                const float maxDistance = 1.2f * dmax, minDistance = 0.8f * dmin;   // GetMax / GetMinDistanceInvariance
                if (!(dist < minDistance || dist > maxDistance)) {          // :236-237
                    double dot = 0.0;
                    for (int k = 0; k < 3; k++) dot += (double)PO[k] * (double)L.mpNormal[3 * jj + k];   // Mat::dot: double accumulation
                    const float viewCos = (float)(dot / (double)dist);     // :242
                    if (!(viewCos < L.viewCosLimit)) {                      // :244-245
                        in = 1;
                        t.proj_x = u;
                        t.proj_xr = u - P.prm.bf * invz;
                        t.proj_y = v;
                        t.scale_level = predict_scale(dmax, dist, L.logScale, P.prm.nlevels);
                        t.view_cos = viewCos;
                    }
                }
            }
        }
    }
    L.inView[jj] = in; L.track[jj] = t;
    if (L.inViewOut) L.inViewOut[jj] = in;
    if (L.trackOut) L.trackOut[jj] = t;
}

// Query of an in-view point: window radius RadiusByViewingCos(viewCos) * th * mvScaleFactors[L] (:59-66), levels [L-1, L]
__device__ __forceinline__ bool local_query(const LocalDev &L, size_t jj, Query &Q) {
    const msl_local_track t = L.track[jj];
    float r = ((double)t.view_cos > 0.998) ? 2.5f : 4.0f;                // float vs double constant, as in the reference
    if (L.m.prm.th != 1.0f) r *= L.m.prm.th;                              // bFactor
    const float radius = r * L.m.prm.scale_factors[t.scale_level];
    Q.u = t.proj_x; Q.v = t.proj_y; Q.ur = t.proj_xr; Q.radius = radius;
    Q.minLevel = t.scale_level - 1; Q.maxLevel = t.scale_level;
    return grid_window(L.m, Q.u, Q.v, radius, Q);
}

// ---- k_local_candidates: one wave per local map point ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_local_candidates(LocalDev L) {
    __shared__ unsigned s_cnt[4];
    const int f = blockIdx.y, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + wv;
    if (j >= min(L.nLocal[f], L.mcap)) return;
    const size_t jj = (size_t)f * L.mcap + j;
    if (lane == 0) s_cnt[wv] = 0;
    __builtin_amdgcn_wave_barrier();
    Query Q;
    if (!L.inView[jj] || !local_query(L, jj, Q)) {
        if (lane == 0) L.m.candCnt[jj] = 0;
        return;
    }
    wave_candidates(L.m, f, Q, L.mpDesc + jj * 32, DIST_BELOW_256, L.m.cand + jj * CMAX, &s_cnt[wv], lane);   // distance 256 never becomes best or second
    if (lane == 0) L.m.candCnt[jj] = s_cnt[wv];
}

// ---- k_local_assign: one workgroup per frame -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LOCAL_NT) void k_local_assign(LocalDev L) {
    extern __shared__ int s_ldyn[];          // t[cap] int | pick[mcap] short
    __shared__ int s_nm, s_ntm;
    const MatchDev &P = L.m;
    const int f = blockIdx.x;
    const int nLoc = min(L.nLocal[f], L.mcap), nCur = min(P.nCur[f], P.cap);
    int *s_t = s_ldyn;
    short *s_pick = reinterpret_cast<short *>(s_ldyn + P.cap);
    const unsigned short *items = P.items + (size_t)f * P.cap;
    const uint8_t *cflags = L.curFlags + (size_t)f * P.cap;
    const uint8_t *mflags = L.mpFlags + (size_t)f * L.mcap;
    const msl_keypoint *kps = P.curKps + (size_t)f * P.cap;
    if (threadIdx.x == 0) s_ntm = 0;

    // point j's choice given the current t: best and second-best key over the candidates it does not skip, then :106-112
    auto pick_of = [&](int j) -> int {
        const size_t jj = (size_t)f * L.mcap + j;
        unsigned b1 = KEY_NONE, b2 = KEY_NONE;
        unskipped_candidates(P, f, jj, j, L.mpDesc + jj * 32, DIST_BELOW_256, s_t, [&](Query &Q) { return local_query(L, jj, Q); },
                             [&](unsigned key) { two_smallest(key, b1, b2); });
        if (b1 == KEY_NONE) return -1;
        const int bestDist = (int)(b1 >> 16);
        if (bestDist > TH_HIGH) return -1;                                 // :106
        const int bestLevel = kps[items[b1 & 0xFFFFu]].octave;
        const int bestLevel2 = b2 == KEY_NONE ? -1 : kps[items[b2 & 0xFFFFu]].octave;
        const int bestDist2 = b2 == KEY_NONE ? 256 : (int)(b2 >> 16);
        if (bestLevel == bestLevel2 && (float)bestDist > L.nnRatio * (float)bestDist2) return -1;   // :107-108
        return (int)items[b1 & 0xFFFFu];
    };
    // keypoints pre-held with observations (cur_flags 3) are skipped by every point
    greedy_assign<LOCAL_NT>(nLoc, nCur, s_t, s_pick, &s_nm, pick_of, [&](int j) { return (mflags[j] & 2) != 0; },
                            [&](int i) { return (cflags[i] & 3) == 3 ? -1 : T_FREE; });
    int ntm = 0;
    for (int j = threadIdx.x; j < nLoc; j += LOCAL_NT) ntm += L.inView[(size_t)f * L.mcap + j];
    if (ntm) atomicAdd(&s_ntm, ntm);
    __syncthreads();
    for (int i = threadIdx.x; i < P.cap; i += LOCAL_NT) P.matchOut[(size_t)f * P.cap + i] = i < nCur ? s_t[i] : -1;
    if (threadIdx.x == 0) { P.nmatches[f] = s_nm; L.nToMatch[f] = s_ntm; }
}

__global__ void k_descriptor_distance(const uint8_t *a, const uint8_t *b, int n, int32_t *out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint4 a0, a1, b0, b1;
    load_desc(a + (size_t)i * 32, a0, a1);
    load_desc(b + (size_t)i * 32, b0, b1);
    out[i] = hamming256(a0, a1, b0, b1);
}

constexpr const char *WHO_PROJECTION = "msl_match_by_projection", *WHO_LOCAL = "msl_match_local_points";

int check_projection(int n_pairs, int cap, const msl_match_params *params, const msl_keypoint *cur_kps, const float *cur_un_xy, const float *cur_uright,
                     const int32_t *cur_grid_cell, const uint8_t *cur_desc, const int32_t *n_cur, const float *last_xyz, const uint8_t *last_desc,
                     const uint8_t *last_flags, const int32_t *last_octave, const float *last_angle, const int32_t *n_last, const float *Tcw_cur,
                     const float *Tcw_last, msl_mem, int32_t *match_out, int32_t *nmatches, msl_mem) {
    const char *who = WHO_PROJECTION;
    if (!none_null(who, {MSL_NAMED(params), MSL_NAMED(cur_kps), MSL_NAMED(cur_un_xy), MSL_NAMED(cur_uright), MSL_NAMED(cur_grid_cell),
                         MSL_NAMED(cur_desc), MSL_NAMED(n_cur), MSL_NAMED(last_xyz), MSL_NAMED(last_desc), MSL_NAMED(last_flags),
                         MSL_NAMED(last_octave), MSL_NAMED(last_angle), MSL_NAMED(n_last), MSL_NAMED(Tcw_cur), MSL_NAMED(Tcw_last),
                         MSL_NAMED(match_out), MSL_NAMED(nmatches)})) return MSL_ERR_INVALID;
    if (!at_least_one(who, "n_pairs", n_pairs) || !in_range(who, "cap", cap, 1, MAX_CAP) || !frame_ok(who, *params)) return MSL_ERR_INVALID;
    return MSL_OK;
}

int launch_projection(msl_match *h, int n_pairs, int cap, const msl_match_params *params, const msl_keypoint *cur_kps, const float *cur_un_xy,
                      const float *cur_uright, const int32_t *cur_grid_cell, const uint8_t *cur_desc, const int32_t *n_cur, const float *last_xyz,
                      const uint8_t *last_desc, const uint8_t *last_flags, const int32_t *last_octave, const float *last_angle, const int32_t *n_last,
                      const float *Tcw_cur, const float *Tcw_last, msl_mem mem, int32_t *match_out, int32_t *nmatches, msl_mem out_mem) {
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    hipStream_t st = h->stream;
    const size_t F = (size_t)n_pairs, n = F * cap;
    Stage S(h, mem, out_mem);
    MatchDev P{};
    stage_current_frame(S, P, n_pairs, cap, *params, cur_kps, cur_un_xy, cur_uright, cur_grid_cell, cur_desc, n_cur);
    P.mb = params->bf / params->fx;                                                                  // :150
    P.lastXyz = S.in(last_xyz, 3 * n); P.lastDesc = S.in(last_desc, 32 * n); P.lastFlags = S.in(last_flags, n); P.lastOctave = S.in(last_octave, n);
    P.lastAngle = S.in(last_angle, n); P.nLast = S.in(n_last, F); P.TcwCur = S.in(Tcw_cur, 12 * F); P.TcwLast = S.in(Tcw_last, 12 * F);
    P.matchOut = S.out(match_out, n); P.nmatches = S.out(nmatches, F);
    MSL_HIP_TRY(S.error());
    MSL_HIP_TRY(grow_all(st, {{h->items, sizeof(unsigned short) * n}, {h->cellStart, sizeof(unsigned) * (NCELLS + 1) * n_pairs},
                              {h->mode, sizeof(int) * n_pairs}, {h->cand, sizeof(unsigned) * CMAX * n}, {h->candCnt, sizeof(unsigned) * n}}));
    P.items = (unsigned short *)h->items.p; P.cellStart = (unsigned *)h->cellStart.p; P.mode = (int *)h->mode.p; P.cand = (unsigned *)h->cand.p;
    P.candCnt = (unsigned *)h->candCnt.p;
    MSL_HIP_TRY(allow_lds(h, LDS_MATCH_ASSIGN, k_match_assign, 3 * sizeof(int) * MAX_CAP));
    hipLaunchKernelGGL(k_match_grid, dim3((unsigned)n_pairs), dim3(256), sizeof(unsigned short) * cap, st, P);
    hipLaunchKernelGGL(k_match_candidates, dim3((unsigned)((cap + 3) / 4), (unsigned)n_pairs), dim3(256), 0, st, P);
    hipLaunchKernelGGL(k_match_assign, dim3((unsigned)n_pairs), dim3(ASSIGN_NT), 3 * sizeof(int) * cap, st, P);
    MSL_HIP_TRY(hipGetLastError());
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}

int check_local(int n_frames, int cap, int mcap, const msl_local_match_params *params, const msl_keypoint *cur_kps, const float *cur_un_xy,
                const float *cur_uright, const int32_t *cur_grid_cell, const uint8_t *cur_desc, const int32_t *n_cur, const uint8_t *cur_flags,
                const float *mp_xyz, const float *mp_normal, const float *mp_dist, const uint8_t *mp_desc, const uint8_t *mp_flags, const int32_t *n_local,
                const float *Tcw, msl_mem, int32_t *match_out, int32_t *n_to_match, int32_t *nmatches, uint8_t *, msl_local_track *, msl_mem) {
    const char *who = WHO_LOCAL;
    if (!none_null(who, {MSL_NAMED(params), MSL_NAMED(cur_kps), MSL_NAMED(cur_un_xy), MSL_NAMED(cur_uright), MSL_NAMED(cur_grid_cell),
                         MSL_NAMED(cur_desc), MSL_NAMED(n_cur), MSL_NAMED(cur_flags), MSL_NAMED(mp_xyz), MSL_NAMED(mp_normal), MSL_NAMED(mp_dist),
                         MSL_NAMED(mp_desc), MSL_NAMED(mp_flags), MSL_NAMED(n_local), MSL_NAMED(Tcw), MSL_NAMED(match_out), MSL_NAMED(n_to_match),
                         MSL_NAMED(nmatches)})) return MSL_ERR_INVALID;   // in_view and track are optional
    if (!at_least_one(who, "n_frames", n_frames) || !in_range(who, "cap", cap, 1, MAX_CAP) || !in_range(who, "mcap", mcap, 1, MAX_MCAP) ||
        !frame_ok(who, params->base) || !log_scale_ok(who, params->log_scale_factor)) return MSL_ERR_INVALID;
    return MSL_OK;
}

int launch_local(msl_match *h, int n_frames, int cap, int mcap, const msl_local_match_params *lp, const msl_keypoint *cur_kps, const float *cur_un_xy,
                 const float *cur_uright, const int32_t *cur_grid_cell, const uint8_t *cur_desc, const int32_t *n_cur, const uint8_t *cur_flags,
                 const float *mp_xyz, const float *mp_normal, const float *mp_dist, const uint8_t *mp_desc, const uint8_t *mp_flags, const int32_t *n_local,
                 const float *Tcw, msl_mem mem, int32_t *match_out, int32_t *n_to_match, int32_t *nmatches, uint8_t *in_view, msl_local_track *track,
                 msl_mem out_mem) {
    const msl_match_params *params = &lp->base;
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    hipStream_t st = h->stream;
    const size_t n = (size_t)n_frames * cap, m = (size_t)n_frames * mcap, F = (size_t)n_frames;
    Stage S(h, mem, out_mem);
    LocalDev L{};
    MatchDev &P = L.m;
    stage_current_frame(S, P, n_frames, cap, *params, cur_kps, cur_un_xy, cur_uright, cur_grid_cell, cur_desc, n_cur);
    L.mcap = mcap; L.logScale = lp->log_scale_factor; L.viewCosLimit = lp->view_cos_limit; L.nnRatio = lp->nn_ratio;
    L.curFlags = S.in(cur_flags, n); L.mpXyz = S.in(mp_xyz, 3 * m); L.mpNormal = S.in(mp_normal, 3 * m); L.mpDist = S.in(mp_dist, 2 * m);
    L.mpDesc = S.in(mp_desc, 32 * m); L.mpFlags = S.in(mp_flags, m); L.nLocal = S.in(n_local, F); P.TcwCur = S.in(Tcw, 12 * F);
    P.matchOut = S.out(match_out, n); P.nmatches = S.out(nmatches, F); L.nToMatch = S.out(n_to_match, F);
    MSL_HIP_TRY(S.error());
    MSL_HIP_TRY(grow_all(st, {{h->items, sizeof(unsigned short) * n}, {h->cellStart, sizeof(unsigned) * (NCELLS + 1) * F},
                              {h->cand, sizeof(unsigned) * CMAX * m}, {h->candCnt, sizeof(unsigned) * m}, {h->trk, sizeof(msl_local_track) * m},
                              {h->inView, m}}));
    P.items = (unsigned short *)h->items.p; P.cellStart = (unsigned *)h->cellStart.p; P.cand = (unsigned *)h->cand.p; P.candCnt = (unsigned *)h->candCnt.p;
    P.mode = nullptr;
    L.track = (msl_local_track *)h->trk.p; L.inView = (uint8_t *)h->inView.p;
    L.inViewOut = S.out_of_scratch(in_view, L.inView, m); L.trackOut = S.out_of_scratch(track, L.track, m);   // the optional in_view / track
    const size_t lds = sizeof(int) * (size_t)cap + sizeof(short) * (size_t)mcap;   // 96 KB at the limits (see k_local_assign)
    MSL_HIP_TRY(allow_lds(h, LDS_LOCAL_ASSIGN, k_local_assign, sizeof(int) * MAX_CAP + sizeof(short) * MAX_MCAP));
    hipLaunchKernelGGL(k_match_grid, dim3((unsigned)n_frames), dim3(256), sizeof(unsigned short) * cap, st, P);
    hipLaunchKernelGGL(k_local_frustum, dim3((unsigned)((mcap + 255) / 256), (unsigned)n_frames), dim3(256), 0, st, L);
    hipLaunchKernelGGL(k_local_candidates, dim3((unsigned)((mcap + 3) / 4), (unsigned)n_frames), dim3(256), 0, st, L);
    hipLaunchKernelGGL(k_local_assign, dim3((unsigned)n_frames), dim3(LOCAL_NT), lds, st, L);
    MSL_HIP_TRY(hipGetLastError());
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}

int run_distance(msl_match *h, const uint8_t *a32, const uint8_t *b32, int n, int32_t *dist_out) {
    if (!h || n < 0 || (n && (!a32 || !b32 || !dist_out))) { set_error("msl_match_descriptor_distance: invalid argument"); return MSL_ERR_INVALID; }
    if (n == 0) return MSL_OK;
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    Stage S(h, MSL_MEM_HOST, MSL_MEM_HOST);
    const uint8_t *a = S.in(a32, (size_t)n * 32), *b = S.in(b32, (size_t)n * 32);
    int32_t *out = S.out(dist_out, (size_t)n);
    MSL_HIP_TRY(S.error());
    hipLaunchKernelGGL(k_descriptor_distance, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, a, b, n, out);
    MSL_HIP_TRY(hipGetLastError());
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}

}  // namespace

void *msl::Stage::take(void *user, size_t bytes, msl_mem side, bool copy_in, bool back) {
    if (!user || err_ != hipSuccess) return nullptr;
    if (side != MSL_MEM_HOST) return user;
    if (used_ == msl_match::STAGE_SLOTS) { err_ = hipErrorOutOfMemory; return nullptr; }   // an entry point outgrew STAGE_SLOTS
    DevBuf &b = h_->stage[used_++];
    err_ = b.grow(bytes, h_->stream);
    if (err_ == hipSuccess && copy_in) err_ = hipMemcpyAsync(b.p, user, bytes, hipMemcpyHostToDevice, h_->stream);
    if (err_ != hipSuccess) return nullptr;
    if (back) copy_back(user, b.p, bytes);
    return b.p;
}

void msl::Stage::copy_back(void *user, const void *dev, size_t bytes) {
    if (nBack_ == msl_match::STAGE_SLOTS) { err_ = hipErrorOutOfMemory; return; }
    back_[nBack_++] = Back{user, dev, bytes};
}

hipError_t msl::Stage::finish() {
    for (int i = 0; i < nBack_; i++) {
        const hipError_t e = hipMemcpyAsync(back_[i].user, back_[i].dev, back_[i].bytes, hipMemcpyDeviceToHost, h_->stream);
        if (e != hipSuccess) return e;
    }
    return outMem_ == MSL_MEM_HOST || mem_ == MSL_MEM_HOST ? hipStreamSynchronize(h_->stream) : hipSuccess;
}

extern "C" {

msl_match *msl_match_create(int device) noexcept {
    try {
    if (bind_device(device) != MSL_OK) return nullptr;
    msl_match *h = new (std::nothrow) msl_match();
    if (!h) { set_error("msl_match_create: out of memory"); return nullptr; }
    h->device = device;
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { set_error("msl_match_create: hipStreamCreate failed"); delete h; return nullptr; }
    return h;
    } MSL_ABI_CATCH_PTR
}

void msl_match_destroy(msl_match *h) noexcept {
    try {
    if (!h) return;
    (void)bind_device(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    const hipStream_t own = h->ownStream ? h->stream : nullptr;
    delete h;                                    // frees the buffers
    if (own) (void)hipStreamDestroy(own);
    } MSL_ABI_CATCH_VOID
}

int msl_match_set_stream(msl_match *h, void *hip_stream) noexcept {
    try {
    if (!h) { set_error("msl_match_set_stream: null handle"); return MSL_ERR_INVALID; }
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    MSL_HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->ownStream && h->stream) (void)hipStreamDestroy(h->stream);
    h->stream = (hipStream_t)hip_stream; h->ownStream = false;
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}

int msl_match_sync(msl_match *h) noexcept {
    try {
    if (!h) { set_error("msl_match_sync: null handle"); return MSL_ERR_INVALID; }
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    MSL_HIP_TRY(hipStreamSynchronize(h->stream));
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}

int msl_match_by_projection(msl_match *h, int n_pairs, int cap, const msl_match_params *params, const msl_keypoint *cur_kps,
                            const float *cur_un_xy, const float *cur_uright, const int32_t *cur_grid_cell, const uint8_t *cur_desc,
                            const int32_t *n_cur, const float *last_xyz, const uint8_t *last_desc, const uint8_t *last_flags,
                            const int32_t *last_octave, const float *last_angle, const int32_t *n_last, const float *Tcw_cur,
                            const float *Tcw_last, msl_mem mem, int32_t *match_out, int32_t *nmatches, msl_mem out_mem) noexcept {
    try {
    return handle_form(WHO_PROJECTION, check_projection, launch_projection, h, n_pairs, cap, params, cur_kps, cur_un_xy, cur_uright, cur_grid_cell, cur_desc,
                       n_cur, last_xyz, last_desc, last_flags, last_octave, last_angle, n_last, Tcw_cur, Tcw_last, mem, match_out, nmatches, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_match_descriptor_distances(msl_match *h, const uint8_t *a32, const uint8_t *b32, int n, int32_t *dist_out) noexcept {
    try {
    return run_distance(h, a32, b32, n, dist_out);
    } MSL_ABI_CATCH_INT
}

int msl_match_by_projection_batch(int device, int n_pairs, int cap, const msl_match_params *params, const msl_keypoint *cur_kps,
                                  const float *cur_un_xy, const float *cur_uright, const int32_t *cur_grid_cell, const uint8_t *cur_desc,
                                  const int32_t *n_cur, const float *last_xyz, const uint8_t *last_desc, const uint8_t *last_flags,
                                  const int32_t *last_octave, const float *last_angle, const int32_t *n_last, const float *Tcw_cur,
                                  const float *Tcw_last, msl_mem mem, int32_t *match_out, int32_t *nmatches, msl_mem out_mem) noexcept {
    try {
    return batch_form(check_projection, launch_projection, device, mem == MSL_MEM_DEVICE, n_pairs, cap, params, cur_kps, cur_un_xy, cur_uright, cur_grid_cell,
                      cur_desc, n_cur, last_xyz, last_desc, last_flags, last_octave, last_angle, n_last, Tcw_cur, Tcw_last, mem, match_out, nmatches, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_match_local_points(msl_match *h, int n_frames, int cap, int mcap, const msl_local_match_params *params, const msl_keypoint *cur_kps,
                           const float *cur_un_xy, const float *cur_uright, const int32_t *cur_grid_cell, const uint8_t *cur_desc, const int32_t *n_cur,
                           const uint8_t *cur_flags, const float *mp_xyz, const float *mp_normal, const float *mp_dist, const uint8_t *mp_desc,
                           const uint8_t *mp_flags, const int32_t *n_local, const float *Tcw, msl_mem mem, int32_t *match_out, int32_t *n_to_match,
                           int32_t *nmatches, uint8_t *in_view, msl_local_track *track, msl_mem out_mem) noexcept {
    try {
    return handle_form(WHO_LOCAL, check_local, launch_local, h, n_frames, cap, mcap, params, cur_kps, cur_un_xy, cur_uright, cur_grid_cell, cur_desc, n_cur,
                       cur_flags, mp_xyz, mp_normal, mp_dist, mp_desc, mp_flags, n_local, Tcw, mem, match_out, n_to_match, nmatches, in_view, track, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_match_local_points_batch(int device, int n_frames, int cap, int mcap, const msl_local_match_params *params, const msl_keypoint *cur_kps,
                                 const float *cur_un_xy, const float *cur_uright, const int32_t *cur_grid_cell, const uint8_t *cur_desc,
                                 const int32_t *n_cur, const uint8_t *cur_flags, const float *mp_xyz, const float *mp_normal, const float *mp_dist,
                                 const uint8_t *mp_desc, const uint8_t *mp_flags, const int32_t *n_local, const float *Tcw, msl_mem mem,
                                 int32_t *match_out, int32_t *n_to_match, int32_t *nmatches, uint8_t *in_view, msl_local_track *track,
                                 msl_mem out_mem) noexcept {
    try {
    return batch_form(check_local, launch_local, device, mem == MSL_MEM_DEVICE, n_frames, cap, mcap, params, cur_kps, cur_un_xy, cur_uright, cur_grid_cell,
                      cur_desc, n_cur, cur_flags, mp_xyz, mp_normal, mp_dist, mp_desc, mp_flags, n_local, Tcw, mem, match_out, n_to_match, nmatches, in_view,
                      track, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_match_descriptor_distance(int device, const uint8_t *a32, const uint8_t *b32, int n, int32_t *dist_out) noexcept {
    try {
    return abi_call_default(run_distance, device, false, a32, b32, n, dist_out);
    } MSL_ABI_CATCH_INT
}

}  // extern "C"

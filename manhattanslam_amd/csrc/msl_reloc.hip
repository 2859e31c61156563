// msl_reloc.hip -- the keyframe search of Tracking::Relocalization for gfx950, batched over independent (frame, keyframe) pairs.
//
// Replaces ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*> &sAlreadyFound, th, ORBdist)
// (reference src/ORBmatcher.cc:680-797): the coarse (th 10, ORBdist 100) and narrow (th 3, ORBdist 64) window searches that run between
// the pose optimisations of a relocalisation (src/Tracking.cc:1990-2035).
//
// Pair-batched (blockIdx.y / blockIdx.x = pair), three launches per call, the first of them k_match_grid (msl_match_window.h, no last
// frame: mode == nullptr):
//   k_kf_candidates   one wave per keyframe point: lane-uniform projection (:702-715, no positive-depth test), cv::norm distance and the
//                     invariance range (:718-726), MapPoint::PredictScale (src/MapPoint.cc:350-364), then the window of radius
//                     th * mvScaleFactors[level] over levels [level-1, level+1] spread over the lanes exactly as the last-frame search
//                     does (wave_candidates without the mvuRight test); candidates go to the handle's cand / candCnt scratch;
//   k_kf_assign       one workgroup per pair: the sequential hand-out of :744-761 (a keypoint held on entry or taken by an earlier
//                     keyframe point is skipped, nothing is overwritten) as the min-fixpoint of msl_assign.h with has_obs == true and
//                     seed_t(i) = cur_held[i] ? -1 : T_FREE, then the rotation histogram, the three maxima and the NULLing (:763-794).
// Distance 256 never becomes best (dist < bestDist from 256, :753), so candidates are kept below it; the pick is the smallest
// (dist << 16 | item position) key, i.e. the first minimum in walk order, accepted when its distance is <= orb_dist (:759).
// LDS of k_kf_assign: t[cap] int + pick[kcap] short = 48 KB at the limits (cap = kcap = 8192).
#include "msl_assign.h"
#include "msl_match_handle.h"
#include "msl_match_math.h"
#include "msl_match_window.h"

#include <vector>

using namespace msl;

// ==== KeyFrameDatabase on one device (reference src/KeyFrameDatabase.cc) ========================================================================
// One slot per added keyframe, in add order, never reused before clear: the slot is the keyframe's position in every inverted list of
// the reference.  Storage is CSR (offsets per slot, ascending words, values); words / values grow geometrically.  `mutex` serialises add,
// erase, clear and the enqueueing of a query (the reference's mMutex).  `lastQuery` is recorded behind every query: the next query's
// stream waits for it (consecutive queries see each other's mRelocScore), and add / erase / clear wait for it on the host before they
// touch or move the storage, so no query in flight reads freed or half-written memory.  The database's own copies and fills run on
// `stream` (non-blocking) and are waited for there before add / erase / clear return: nothing but that stream, the last query and, for a
// device-memory add, the producing handle's stream is ever waited for.
struct msl_kfdb {
    static constexpr int MAX_SLOTS = 8192;
    int device = 0;
    std::mutex mutex;
    hipStream_t stream = nullptr;
    hipEvent_t lastQuery = nullptr;
    bool queried = false;
    DevBuf words, values;                       // [usedCap] int32 / double
    DevBuf offsets, live, score;                // [MAX_SLOTS + 1] int32, [MAX_SLOTS] uint8, [MAX_SLOTS] float (mRelocScore, kept across queries)
    std::vector<int> hostOffsets{0};
    std::vector<uint8_t> hostLive;
    int nLive = 0;
};

namespace {

constexpr int MAX_KCAP = 8192;                  // map points of the keyframe of a pair (msl_pnp.hip has a kcap of its own)
constexpr int KF_NT = 1024;

struct KfDev {
    MatchDev m;                                     // current frame, grid scratch, candidates (per keyframe point), params (m.prm = base), TcwCur, outputs
    int kcap, orbDist;
    float logScale;
    const uint8_t *curHeld;
    const float *kfXyz, *kfDist, *kfAngle; const uint8_t *kfDesc, *kfFlags; const int32_t *nKf;
};

// Projection of keyframe point q into the current frame (:702-734): false = the point matches nothing.
__device__ __forceinline__ bool kf_query(const KfDev &K, int pair, size_t qi, Query &Q) {
    const MatchDev &P = K.m;
    const float *Tc = P.TcwCur + (size_t)pair * 12;
    const float tcw[3] = {Tc[3], Tc[7], Tc[11]};
    const float x3Dw[3] = {K.kfXyz[3 * qi], K.kfXyz[3 * qi + 1], K.kfXyz[3 * qi + 2]};
    float x3Dc[3];
    gemm3(Tc, false, 1.0, x3Dw, tcw, x3Dc);                             // x3Dc = Rcw * x3Dw + tcw (:703)
    const float xc = x3Dc[0], yc = x3Dc[1];
    const float invzc = (float)(1.0 / (double)x3Dc[2]);                 // :707, no sign test
    const float u = P.prm.fx * xc * invzc + P.prm.cx;                   // :709-710, left to right
    const float v = P.prm.fy * yc * invzc + P.prm.cy;
    if (!(u >= P.prm.minX && u <= P.prm.maxX)) return false;            // :712-715; a NaN (zc == 0) matches nothing
    if (!(v >= P.prm.minY && v <= P.prm.maxY)) return false;
    float Ow[3];
    gemm3(Tc, true, -1.0, tcw, nullptr, Ow);                            // Ow = -Rcw.t() * tcw (:686)
    const float PO[3] = {x3Dw[0] - Ow[0], x3Dw[1] - Ow[1], x3Dw[2] - Ow[2]};
    double ss = 0.0;
    for (int k = 0; k < 3; k++) ss += (double)PO[k] * (double)PO[k];
    const float dist3D = (float)sqrt(ss);                               // cv::norm on CV_32F (:719)
    const float dmin = K.kfDist[2 * qi], dmax = K.kfDist[2 * qi + 1];
    const float maxDistance = 1.2f * dmax, minDistance = 0.8f * dmin;   // GetMax / GetMinDistanceInvariance
    if (dist3D < minDistance || dist3D > maxDistance) return false;     // :725
    const int level = predict_scale(dmax, dist3D, K.logScale, P.prm.nlevels);   // :728
    const float radius = P.prm.th * P.prm.scale_factors[level];         // :731
    Q.u = u; Q.v = v; Q.ur = 0.0f; Q.radius = radius;
    Q.minLevel = level - 1; Q.maxLevel = level + 1;                     // :733
    return grid_window(P, u, v, radius, Q);
}

// ---- k_kf_candidates: one wave per keyframe point -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_kf_candidates(KfDev K) {
    __shared__ unsigned s_cnt[4];
    const int pair = blockIdx.y, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + wv;
    if (q >= min(K.nKf[pair], K.kcap)) return;
    const size_t qi = (size_t)pair * K.kcap + q;
    if (lane == 0) s_cnt[wv] = 0;
    __builtin_amdgcn_wave_barrier();
    Query Q;
    if (!(K.kfFlags[qi] & 1) || !kf_query(K, pair, qi, Q)) {
        if (lane == 0) K.m.candCnt[qi] = 0;
        return;
    }
    wave_candidates<false>(K.m, pair, Q, K.kfDesc + qi * 32, DIST_BELOW_256, K.m.cand + qi * CMAX, &s_cnt[wv], lane);
    if (lane == 0) K.m.candCnt[qi] = s_cnt[wv];
}

// ---- k_kf_assign: one workgroup per pair ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KF_NT) void k_kf_assign(KfDev K) {
    extern __shared__ int s_kdyn[];         // t[cap] int | pick[kcap] short
    __shared__ int s_hist[ROT_HISTO_LENGTH], s_keep[3], s_nm;
    const MatchDev &P = K.m;
    const int pair = blockIdx.x;
    const int nKf = min(K.nKf[pair], K.kcap), nCur = min(P.nCur[pair], P.cap);
    int *s_t = s_kdyn;
    short *s_pick = reinterpret_cast<short *>(s_kdyn + P.cap);
    const unsigned short *items = P.items + (size_t)pair * P.cap;
    const size_t base = (size_t)pair * P.cap, kbase = (size_t)pair * K.kcap;
    const uint8_t *held = K.curHeld + base;
    if (threadIdx.x < ROT_HISTO_LENGTH) s_hist[threadIdx.x] = 0;

    // keyframe point q's choice given the current t: the first minimum in walk order over the keypoints it does not skip, bestDist <= ORBdist (:759)
    auto pick_of = [&](int q) -> int {
        unsigned best = KEY_NONE;
        unskipped_candidates<false>(P, pair, kbase + q, q, K.kfDesc + (kbase + q) * 32, DIST_BELOW_256, s_t,
                                    [&](Query &Q) { return kf_query(K, pair, kbase + q, Q); }, [&](unsigned key) { best = min(best, key); });
        return (best != KEY_NONE && (int)(best >> 16) <= K.orbDist) ? (int)items[best & 0xFFFFu] : -1;
    };
    // :746-747: a held keypoint is skipped by every query, and every accepted pick holds its keypoint from then on
    greedy_assign<KF_NT>(nKf, nCur, s_t, s_pick, &s_nm, pick_of, [](int) { return true; }, [&](int i) { return held[i] ? -1 : T_FREE; });
    if (P.prm.check_orientation) {          // rotation histogram, three maxima, NULLing (:763-794)
        rotation_cull<KF_NT>(nKf, s_hist, s_keep,
                             [&](int q) { return s_pick[q] >= 0 ? rot_bin(K.kfAngle[kbase + q] - P.curKps[base + s_pick[q]].angle) : -1; },
                             [&](int q) {
                                 s_t[s_pick[q]] = -1;
                                 atomicSub(&s_nm, 1);
                             });
    }
    for (int i = threadIdx.x; i < P.cap; i += KF_NT) P.matchOut[base + i] = i < nCur ? s_t[i] : -1;
    if (threadIdx.x == 0) P.nmatches[pair] = s_nm;
}

constexpr const char *WHO_KEYFRAME = "msl_match_keyframe_points", *WHO_RELOC = "msl_reloc_candidates";

int check_keyframe(int n_pairs, int cap, int kcap, const msl_keyframe_match_params *params, const msl_keypoint *cur_kps, const float *cur_un_xy,
                   const int32_t *cur_grid_cell, const uint8_t *cur_desc, const int32_t *n_cur, const uint8_t *cur_held, const float *kf_xyz,
                   const float *kf_dist, const uint8_t *kf_desc, const float *kf_angle, const uint8_t *kf_flags, const int32_t *n_kf, const float *Tcw,
                   msl_mem, int32_t *match_out, int32_t *nmatches, msl_mem) {
    const char *who = WHO_KEYFRAME;
    if (!none_null(who, {MSL_NAMED(params), MSL_NAMED(cur_kps), MSL_NAMED(cur_un_xy), MSL_NAMED(cur_grid_cell), MSL_NAMED(cur_desc), MSL_NAMED(n_cur),
                         MSL_NAMED(cur_held), MSL_NAMED(kf_xyz), MSL_NAMED(kf_dist), MSL_NAMED(kf_desc), MSL_NAMED(kf_angle), MSL_NAMED(kf_flags),
                         MSL_NAMED(n_kf), MSL_NAMED(Tcw), MSL_NAMED(match_out), MSL_NAMED(nmatches)})) return MSL_ERR_INVALID;
    if (!at_least_one(who, "n_pairs", n_pairs) || !in_range(who, "cap", cap, 1, MAX_CAP) || !in_range(who, "kcap", kcap, 1, MAX_KCAP) ||
        !frame_ok(who, params->base) || !log_scale_ok(who, params->log_scale_factor) || !in_range(who, "orb_dist", params->orb_dist, 0, 255))
        return MSL_ERR_INVALID;
    return MSL_OK;
}

int launch_keyframe(msl_match *h, int n_pairs, int cap, int kcap, const msl_keyframe_match_params *kp, const msl_keypoint *cur_kps,
                    const float *cur_un_xy, const int32_t *cur_grid_cell, const uint8_t *cur_desc, const int32_t *n_cur, const uint8_t *cur_held,
                    const float *kf_xyz, const float *kf_dist, const uint8_t *kf_desc, const float *kf_angle, const uint8_t *kf_flags, const int32_t *n_kf,
                    const float *Tcw, msl_mem mem, int32_t *match_out, int32_t *nmatches, msl_mem out_mem) {
    const msl_match_params *params = &kp->base;
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    hipStream_t st = h->stream;
    const size_t n = (size_t)n_pairs * cap, m = (size_t)n_pairs * kcap, F = (size_t)n_pairs;
    Stage S(h, mem, out_mem);
    KfDev K{};
    MatchDev &P = K.m;
    stage_current_frame(S, P, n_pairs, cap, *params, cur_kps, cur_un_xy, nullptr, cur_grid_cell, cur_desc, n_cur);   // no mvuRight in this search
    K.kcap = kcap; K.orbDist = kp->orb_dist; K.logScale = kp->log_scale_factor;
    K.curHeld = S.in(cur_held, n); K.kfXyz = S.in(kf_xyz, 3 * m); K.kfDist = S.in(kf_dist, 2 * m); K.kfDesc = S.in(kf_desc, 32 * m);
    K.kfAngle = S.in(kf_angle, m); K.kfFlags = S.in(kf_flags, m); K.nKf = S.in(n_kf, F); P.TcwCur = S.in(Tcw, 12 * F);
    P.matchOut = S.out(match_out, n); P.nmatches = S.out(nmatches, F);
    MSL_HIP_TRY(S.error());
    MSL_HIP_TRY(grow_all(st, {{h->items, sizeof(unsigned short) * n}, {h->cellStart, sizeof(unsigned) * (NCELLS + 1) * F},
                              {h->cand, sizeof(unsigned) * CMAX * m}, {h->candCnt, sizeof(unsigned) * m}}));
    P.items = (unsigned short *)h->items.p; P.cellStart = (unsigned *)h->cellStart.p; P.cand = (unsigned *)h->cand.p; P.candCnt = (unsigned *)h->candCnt.p;
    P.mode = nullptr;
    const size_t lds = sizeof(int) * (size_t)cap + sizeof(short) * (size_t)kcap;
    MSL_HIP_TRY(allow_lds(h, LDS_KF_ASSIGN, k_kf_assign, sizeof(int) * MAX_CAP + sizeof(short) * MAX_KCAP));
    hipLaunchKernelGGL(k_match_grid, dim3((unsigned)n_pairs), dim3(256), sizeof(unsigned short) * cap, st, P);
    hipLaunchKernelGGL(k_kf_candidates, dim3((unsigned)((kcap + 3) / 4), (unsigned)n_pairs), dim3(256), 0, st, K);
    hipLaunchKernelGGL(k_kf_assign, dim3((unsigned)n_pairs), dim3(KF_NT), lds, st, K);
    MSL_HIP_TRY(hipGetLastError());
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}


constexpr int MAX_SLOTS = msl_kfdb::MAX_SLOTS;
constexpr int COVIS = 10;                       // GetBestCovisibilityKeyFrames(10)
constexpr int SEL_NT = 1024;

struct RelocDev {
    int nFrames, cap, ccap, nSlots;
    const int32_t *qWord; const double *qValue; const int32_t *qN; const int32_t *covis;
    const int32_t *dbWord; const double *dbValue; const int32_t *dbOff; const uint8_t *dbLive; float *dbScore;
    int32_t *cnt, *first; float *score;         // scratch [nFrames][nSlots]
    int32_t *candOut, *nCand, *wordsOut; float *scoreOut;
};

// ---- k_reloc_score: one wave per (slot, frame) ----------------------------------------------------------------------------------------------
// mnRelocWords, the first shared word and L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68) of one keyframe against one
// query.  Both word lists ascend, so the merge walk of the reference visits the common words in ascending order: each lane looks one
// keyframe word up in the query by binary search, the ballot keeps the order, and the double sum runs over the set lanes one by one.
__global__ __launch_bounds__(256) void k_reloc_score(RelocDev R) {
    const int f = blockIdx.y, s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (s >= R.nSlots) return;
    const size_t o = (size_t)f * R.nSlots + s;
    const int b = R.dbOff[s], e = R.dbLive[s] ? R.dbOff[s + 1] : b;
    const int nq = min(max(R.qN[f], 0), R.cap);
    const int32_t *qw = R.qWord + (size_t)f * R.cap;
    const double *qv = R.qValue + (size_t)f * R.cap;
    double sum = 0.0;
    int count = 0, firstWord = -1;
    for (int i0 = b; i0 < e; i0 += 64) {
        const int i = i0 + lane;
        bool found = false;
        double term = 0.0;
        int w = 0;
        if (i < e) {
            w = R.dbWord[i];
            int lo = 0, hi = nq;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (qw[mid] < w) lo = mid + 1; else hi = mid; }
            if (lo < nq && qw[lo] == w) {
                found = true;
                const double vi = qv[lo], wi = R.dbValue[i];
                term = fabs(vi - wi) - fabs(vi) - fabs(wi);                 // :41
            }
        }
        unsigned long long mask = __ballot(found);
        if (mask && firstWord < 0) firstWord = __shfl(w, __ffsll((long long)mask) - 1);
        count += __popcll(mask);
        while (mask) {                                                       // in ascending word order, one addition each
            const int src = __ffsll((long long)mask) - 1;
            sum += __shfl(term, src);
            mask &= mask - 1;
        }
    }
    if (lane == 0) {
        R.cnt[o] = count; R.first[o] = firstWord;
        R.score[o] = (float)(-sum / 2.0);                                   // :65, rounded to float on assignment to si
    }
}

// ---- k_reloc_select: one workgroup, the frames of the call in order ---------------------------------------------------------------------
// KeyFrameDatabase::DetectRelocalizationCandidates (src/KeyFrameDatabase.cc:90-169) after the inverted-file walk.  lKFsSharingWords is
// ordered by (first shared word, slot); the scored keyframes keep that order (a bitonic sort of 64-bit keys in LDS), the accumulation over
// the covisible neighbours runs per entry in float, the retained pBestKFs are emitted at their first occurrence (a first-occurrence table
// and an ordered scan).  mRelocScore lives in the database across frames and calls.
__global__ __launch_bounds__(SEL_NT) void k_reloc_select(RelocDev R) {
    extern __shared__ unsigned long long s_key[];      // [N] keys, later int first[N]
    __shared__ unsigned s_wave[17];
    __shared__ int s_max, s_bestAcc;
    const int nS = R.nSlots;
    int N = 1;
    while (N < nS) N <<= 1;
    float *s_acc = reinterpret_cast<float *>(s_key + N);
    unsigned short *s_best = reinterpret_cast<unsigned short *>(s_acc + N);
    int *s_first = reinterpret_cast<int *>(s_key);
    for (int f = 0; f < R.nFrames; f++) {
        const size_t o = (size_t)f * nS;
        if (threadIdx.x == 0) { s_max = 0; s_bestAcc = 0; }
        __syncthreads();
        int mx = 0;
        for (int s = threadIdx.x; s < nS; s += SEL_NT) mx = max(mx, R.cnt[o + s]);
        if (mx) atomicMax(&s_max, mx);
        __syncthreads();
        const int maxCommonWords = s_max;
        const int minCommonWords = (int)((float)maxCommonWords * 0.8f);       // :101
        for (int i = threadIdx.x; i < N; i += SEL_NT) {
            unsigned long long key = ~0ull;
            if (i < nS) {
                const int c = R.cnt[o + i];
                const bool scored = c > 0 && c > minCommonWords;               // :112
                if (scored) {
                    R.dbScore[i] = R.score[o + i];                             // :115
                    key = ((unsigned long long)(unsigned)R.first[o + i] << 13) | (unsigned)i;
                }
                if (R.wordsOut) R.wordsOut[o + i] = c;
                if (R.scoreOut) R.scoreOut[o + i] = scored ? R.score[o + i] : -1.0f;
            }
            s_key[i] = key;
        }
        __syncthreads();
        for (int k = 2; k <= N; k <<= 1)                                        // bitonic sort, ascending
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = threadIdx.x; i < N; i += SEL_NT) {
                    const int p = i ^ j;
                    if (p > i) {
                        const unsigned long long a = s_key[i], b = s_key[p];
                        const bool up = (i & k) == 0;
                        if ((a > b) == up) { s_key[i] = b; s_key[p] = a; }
                    }
                }
                __syncthreads();
            }
        // accumulate score by covisibility (:127-150)
        for (int e = threadIdx.x; e < N; e += SEL_NT) {
            const unsigned long long key = s_key[e];
            float acc = 0.0f;
            int bestKF = 0;
            if (key != ~0ull) {
                const int s = (int)(key & 8191u);
                float bestScore = R.dbScore[s];
                acc = bestScore; bestKF = s;
                for (int k = 0; k < COVIS; k++) {
                    const int n2 = R.covis[(size_t)s * COVIS + k];
                    if (n2 == -1) break;
                    if (n2 < 0 || n2 >= nS || R.cnt[o + n2] == 0) continue;    // mnRelocQuery != F->mnId (:137)
                    const float sc = R.dbScore[n2];
                    acc += sc;                                                  // :140
                    if (sc > bestScore) { bestKF = n2; bestScore = sc; }
                }
                if (acc > 0.0f) atomicMax(&s_bestAcc, __float_as_int(acc));     // :148, bestAccScore starts at 0 (positive floats order as ints)
            }
            s_acc[e] = acc; s_best[e] = (unsigned short)bestKF;
        }
        __syncthreads();
        // s_key is dead from here: its storage becomes the first-occurrence table
        const float minScoreToRetain = 0.75f * __int_as_float(s_bestAcc);       // :153
        bool keep[8];                                                           // entries e = threadIdx.x * per + r, per <= 8
        const int per = (N + SEL_NT - 1) / SEL_NT;
        const int e0 = threadIdx.x * per;
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const int e = e0 + r;
            keep[r] = r < per && e < N && s_key[e] != ~0ull && s_acc[e] > minScoreToRetain;   // :160
        }
        __syncthreads();
        for (int i = threadIdx.x; i < N; i += SEL_NT) s_first[i] = 0x7FFFFFFF;
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 8; r++)
            if (keep[r]) atomicMin(&s_first[s_best[e0 + r]], e0 + r);
        __syncthreads();
        unsigned mine = 0;
#pragma unroll
        for (int r = 0; r < 8; r++) {
            keep[r] = keep[r] && s_first[s_best[e0 + r]] == e0 + r;             // :162, first occurrence only
            mine += keep[r];
        }
        unsigned total;
        unsigned pos = block_excl_scan(mine, s_wave, &total);
#pragma unroll
        for (int r = 0; r < 8; r++)
            if (keep[r]) {
                if ((int)pos < R.ccap) R.candOut[(size_t)f * R.ccap + pos] = s_best[e0 + r];
                pos++;
            }
        if (threadIdx.x == 0) R.nCand[f] = (int)total;
        __syncthreads();
    }
}

const char *const SCORING_NAMES[6] = {"L1_NORM", "L2_NORM", "CHI_SQUARE", "KL", "BHATTACHARYYA", "DOT_PRODUCT"};

// No upper limit on cap or ccap: they size the caller's arrays only.  covis is required once the database holds slots, which
// launch_reloc reads under the database's mutex; words_out and score_out are optional.
int check_reloc(msl_kfdb *db, const msl_vocab *voc, int n_frames, int cap, int ccap, const int32_t *bow_word, const double *bow_value,
                const int32_t *n_words, const int32_t *, msl_mem, int32_t *cand_out, int32_t *n_cand, int32_t *, float *, msl_mem) {
    const char *who = WHO_RELOC;
    if (!none_null(who, {MSL_NAMED(db), MSL_NAMED(voc), MSL_NAMED(bow_word), MSL_NAMED(bow_value), MSL_NAMED(n_words), MSL_NAMED(cand_out),
                         MSL_NAMED(n_cand)})) return MSL_ERR_INVALID;
    if (!at_least_one(who, "n_frames", n_frames) || !at_least_one(who, "cap", cap) || !at_least_one(who, "ccap", ccap)) return MSL_ERR_INVALID;
    return MSL_OK;
}

int launch_reloc(msl_match *h, msl_kfdb *db, const msl_vocab *voc, int n_frames, int cap, int ccap, const int32_t *bow_word, const double *bow_value,
                 const int32_t *n_words, const int32_t *covis, msl_mem mem, int32_t *cand_out, int32_t *n_cand, int32_t *words_out, float *score_out,
                 msl_mem out_mem) {
    int32_t info[7];
    if (msl_vocab_info(voc, info) != MSL_OK) return MSL_ERR_INVALID;
    if (info[2] != 0) {
        set_error("msl_reloc_candidates: only L1_NORM scoring is built; the vocabulary's scoring is %s", info[2] > 0 && info[2] < 6 ? SCORING_NAMES[info[2]] : "unknown");
        return MSL_ERR_INVALID;
    }
    if (info[6] != h->device || db->device != h->device) {
        set_error("msl_reloc_candidates: the vocabulary (device %d) and the database (device %d) must live on the handle's device %d", info[6], db->device,
                  h->device);
        return MSL_ERR_INVALID;
    }
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    std::lock_guard<std::mutex> lock(db->mutex);
    hipStream_t st = h->stream;
    const int nS = (int)db->hostOffsets.size() - 1;
    if (nS > 0 && !covis) { set_error("msl_reloc_candidates: covis is null"); return MSL_ERR_INVALID; }
    const size_t F = (size_t)n_frames, FS = F * (size_t)nS;
    Stage S(h, mem, out_mem);
    RelocDev R{};
    R.nFrames = n_frames; R.cap = cap; R.ccap = ccap; R.nSlots = nS;
    R.qWord = S.in(bow_word, F * cap); R.qValue = S.in(bow_value, F * cap); R.qN = S.in(n_words, F);
    R.covis = nS ? S.in(covis, (size_t)nS * COVIS) : nullptr;
    R.candOut = S.out(cand_out, F * ccap); R.nCand = S.out(n_cand, F);
    R.wordsOut = nS ? S.out(words_out, FS) : nullptr; R.scoreOut = nS ? S.out(score_out, FS) : nullptr;
    MSL_HIP_TRY(S.error());
    MSL_HIP_TRY(grow_all(st, {{h->relocCnt, sizeof(int32_t) * (FS + 1)}, {h->relocFirst, sizeof(int32_t) * (FS + 1)}, {h->relocScore, sizeof(float) * (FS + 1)}}));
    R.cnt = (int32_t *)h->relocCnt.p; R.first = (int32_t *)h->relocFirst.p; R.score = (float *)h->relocScore.p;
    R.dbWord = (const int32_t *)db->words.p; R.dbValue = (const double *)db->values.p; R.dbOff = (const int32_t *)db->offsets.p;
    R.dbLive = (const uint8_t *)db->live.p; R.dbScore = (float *)db->score.p;
    if (db->queried) MSL_HIP_TRY(hipStreamWaitEvent(st, db->lastQuery, 0));   // the previous query's mRelocScore
    int N = 1;
    while (N < nS) N <<= 1;
    const size_t lds = (size_t)N * (sizeof(unsigned long long) + sizeof(float) + sizeof(unsigned short));
    MSL_HIP_TRY(allow_lds(h, LDS_RELOC_SELECT, k_reloc_select, (size_t)MAX_SLOTS * (sizeof(unsigned long long) + sizeof(float) + sizeof(unsigned short))));
    if (nS) hipLaunchKernelGGL(k_reloc_score, dim3((unsigned)((nS + 3) / 4), (unsigned)n_frames), dim3(256), 0, st, R);
    hipLaunchKernelGGL(k_reloc_select, dim3(1), dim3(SEL_NT), lds, st, R);
    const hipError_t launched = hipGetLastError();
    if (hipEventRecord(db->lastQuery, st) == hipSuccess) db->queried = true;     // also behind a failed launch: whatever did start is waited for
    MSL_HIP_TRY(launched);
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}

// add / erase / clear: the queries in flight are done before the storage is touched (mutex held)
hipError_t kfdb_quiesce(msl_kfdb *db) { return db->queried ? hipEventSynchronize(db->lastQuery) : hipSuccess; }

int kfdb_add(msl_kfdb *db, msl_match *h, const int32_t *bow_word, const double *bow_value, const int32_t *n_words, msl_mem mem, int32_t *slot) {
    if (!db || !bow_word || !bow_value || !n_words || !slot || (mem == MSL_MEM_DEVICE && !h) || (h && h->device != db->device)) {
        set_error("msl_kfdb_add: invalid argument (device memory needs the matcher handle that produced it, on the database's device)");
        return MSL_ERR_INVALID;
    }
    int rc = bind_device(db->device);
    if (rc != MSL_OK) return rc;
    std::lock_guard<std::mutex> lock(db->mutex);
    int n = 0;
    if (mem == MSL_MEM_DEVICE) {
        MSL_HIP_TRY(hipStreamSynchronize(h->stream));     // the count is needed on the host: the one wait of a keyframe insertion
        MSL_HIP_TRY(hipMemcpyAsync(&n, n_words, sizeof(int), hipMemcpyDeviceToHost, db->stream));
        MSL_HIP_TRY(hipStreamSynchronize(db->stream));
    } else n = *n_words;
    if (n < 0) { set_error("msl_kfdb_add: negative word count"); return MSL_ERR_INVALID; }
    const int nS = (int)db->hostOffsets.size() - 1;
    if (nS >= MAX_SLOTS) { set_error("msl_kfdb_add: the database holds %d slots already (erased slots come back only at msl_kfdb_clear)", MAX_SLOTS); return MSL_ERR_OVERFLOW; }
    MSL_HIP_TRY(kfdb_quiesce(db));
    const size_t used = (size_t)db->hostOffsets.back(), need = used + (size_t)n;
    if (need * sizeof(double) > db->values.cap) {         // geometric growth: new storage, the old contents copied, then the old freed
        size_t ncap = db->values.cap / sizeof(double) ? db->values.cap / sizeof(double) : 4096;
        while (ncap < need) ncap *= 2;
        DevBuf nw, nv;
        MSL_HIP_TRY(nw.grow(ncap * sizeof(int32_t), db->stream));
        MSL_HIP_TRY(nv.grow(ncap * sizeof(double), db->stream));
        if (used) {
            MSL_HIP_TRY(hipMemcpyAsync(nw.p, db->words.p, used * sizeof(int32_t), hipMemcpyDeviceToDevice, db->stream));
            MSL_HIP_TRY(hipMemcpyAsync(nv.p, db->values.p, used * sizeof(double), hipMemcpyDeviceToDevice, db->stream));
            MSL_HIP_TRY(hipStreamSynchronize(db->stream));        // the old storage is freed by the moves below
        }
        db->words = std::move(nw); db->values = std::move(nv);
    }
    const hipMemcpyKind kind = mem == MSL_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (n) {
        MSL_HIP_TRY(hipMemcpyAsync((int32_t *)db->words.p + used, bow_word, (size_t)n * sizeof(int32_t), kind, db->stream));
        MSL_HIP_TRY(hipMemcpyAsync((double *)db->values.p + used, bow_value, (size_t)n * sizeof(double), kind, db->stream));
    }
    const int end = (int)need;
    const uint8_t one = 1;
    MSL_HIP_TRY(hipMemcpyAsync((int32_t *)db->offsets.p + nS + 1, &end, sizeof(int), hipMemcpyHostToDevice, db->stream));
    MSL_HIP_TRY(hipMemcpyAsync((uint8_t *)db->live.p + nS, &one, 1, hipMemcpyHostToDevice, db->stream));
    MSL_HIP_TRY(hipStreamSynchronize(db->stream));            // the database's own stream only: no other stream of the device is stalled
    db->hostOffsets.push_back(end); db->hostLive.push_back(1); db->nLive++;
    *slot = nS;
    return MSL_OK;
}

int kfdb_erase(msl_kfdb *db, int slot) {
    if (!db) { set_error("msl_kfdb_erase: null database"); return MSL_ERR_INVALID; }
    int rc = bind_device(db->device);
    if (rc != MSL_OK) return rc;
    std::lock_guard<std::mutex> lock(db->mutex);
    if (slot < 0 || slot >= (int)db->hostLive.size() || !db->hostLive[slot]) { set_error("msl_kfdb_erase: slot %d is not a live keyframe", slot); return MSL_ERR_INVALID; }
    MSL_HIP_TRY(kfdb_quiesce(db));
    const uint8_t zero = 0;
    MSL_HIP_TRY(hipMemcpyAsync((uint8_t *)db->live.p + slot, &zero, 1, hipMemcpyHostToDevice, db->stream));
    MSL_HIP_TRY(hipStreamSynchronize(db->stream));
    db->hostLive[slot] = 0; db->nLive--;
    return MSL_OK;
}

int kfdb_clear(msl_kfdb *db) {
    if (!db) { set_error("msl_kfdb_clear: null database"); return MSL_ERR_INVALID; }
    int rc = bind_device(db->device);
    if (rc != MSL_OK) return rc;
    std::lock_guard<std::mutex> lock(db->mutex);
    MSL_HIP_TRY(kfdb_quiesce(db));
    MSL_HIP_TRY(hipMemsetAsync(db->score.p, 0, sizeof(float) * MAX_SLOTS, db->stream));     // new slots hold keyframes never scored
    MSL_HIP_TRY(hipMemsetAsync(db->live.p, 0, MAX_SLOTS, db->stream));
    MSL_HIP_TRY(hipStreamSynchronize(db->stream));
    db->hostOffsets.assign(1, 0); db->hostLive.clear(); db->nLive = 0;
    return MSL_OK;
}

msl_kfdb *kfdb_create(int device) {
    if (bind_device(device) != MSL_OK) return nullptr;
    msl_kfdb *db = new msl_kfdb();
    db->device = device;
    bool ok = hipStreamCreateWithFlags(&db->stream, hipStreamNonBlocking) == hipSuccess;
    const hipStream_t st = db->stream;
    ok = ok && db->offsets.grow(sizeof(int32_t) * (MAX_SLOTS + 1), st) == hipSuccess && db->live.grow(MAX_SLOTS, st) == hipSuccess &&
         db->score.grow(sizeof(float) * MAX_SLOTS, st) == hipSuccess && hipEventCreateWithFlags(&db->lastQuery, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipMemsetAsync(db->offsets.p, 0, sizeof(int32_t) * (MAX_SLOTS + 1), st) == hipSuccess &&
         hipMemsetAsync(db->live.p, 0, MAX_SLOTS, st) == hipSuccess && hipMemsetAsync(db->score.p, 0, sizeof(float) * MAX_SLOTS, st) == hipSuccess &&
         hipStreamSynchronize(st) == hipSuccess;
    if (!ok) {
        set_error("msl_kfdb_create: device allocation failed");
        if (db->lastQuery) (void)hipEventDestroy(db->lastQuery);
        if (db->stream) (void)hipStreamDestroy(db->stream);
        delete db;
        return nullptr;
    }
    return db;
}

}  // namespace

extern "C" {

int msl_match_keyframe_points(msl_match *h, int n_pairs, int cap, int kcap, const msl_keyframe_match_params *params, const msl_keypoint *cur_kps,
                              const float *cur_un_xy, const int32_t *cur_grid_cell, const uint8_t *cur_desc, const int32_t *n_cur, const uint8_t *cur_held,
                              const float *kf_xyz, const float *kf_dist, const uint8_t *kf_desc, const float *kf_angle, const uint8_t *kf_flags,
                              const int32_t *n_kf, const float *Tcw, msl_mem mem, int32_t *match_out, int32_t *nmatches, msl_mem out_mem) noexcept {
    try {
    return handle_form(WHO_KEYFRAME, check_keyframe, launch_keyframe, h, n_pairs, cap, kcap, params, cur_kps, cur_un_xy, cur_grid_cell, cur_desc, n_cur,
                       cur_held, kf_xyz, kf_dist, kf_desc, kf_angle, kf_flags, n_kf, Tcw, mem, match_out, nmatches, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_match_keyframe_points_batch(int device, int n_pairs, int cap, int kcap, const msl_keyframe_match_params *params, const msl_keypoint *cur_kps,
                                    const float *cur_un_xy, const int32_t *cur_grid_cell, const uint8_t *cur_desc, const int32_t *n_cur,
                                    const uint8_t *cur_held, const float *kf_xyz, const float *kf_dist, const uint8_t *kf_desc, const float *kf_angle,
                                    const uint8_t *kf_flags, const int32_t *n_kf, const float *Tcw, msl_mem mem, int32_t *match_out, int32_t *nmatches,
                                    msl_mem out_mem) noexcept {
    try {
    return batch_form(check_keyframe, launch_keyframe, device, mem == MSL_MEM_DEVICE, n_pairs, cap, kcap, params, cur_kps, cur_un_xy, cur_grid_cell, cur_desc,
                      n_cur, cur_held, kf_xyz, kf_dist, kf_desc, kf_angle, kf_flags, n_kf, Tcw, mem, match_out, nmatches, out_mem);
    } MSL_ABI_CATCH_INT
}

msl_kfdb *msl_kfdb_create(int device) noexcept {
    try {
    return kfdb_create(device);
    } MSL_ABI_CATCH_PTR
}

void msl_kfdb_destroy(msl_kfdb *db) noexcept {
    try {
    if (!db) return;
    (void)bind_device(db->device);
    if (db->queried) (void)hipEventSynchronize(db->lastQuery);
    if (db->lastQuery) (void)hipEventDestroy(db->lastQuery);
    if (db->stream) (void)hipStreamDestroy(db->stream);
    delete db;
    } MSL_ABI_CATCH_VOID
}

int msl_kfdb_add(msl_kfdb *db, msl_match *h, const int32_t *bow_word, const double *bow_value, const int32_t *n_words, msl_mem mem,
                 int32_t *slot) noexcept {
    try {
    return kfdb_add(db, h, bow_word, bow_value, n_words, mem, slot);
    } MSL_ABI_CATCH_INT
}

int msl_kfdb_erase(msl_kfdb *db, int slot) noexcept {
    try {
    return kfdb_erase(db, slot);
    } MSL_ABI_CATCH_INT
}

int msl_kfdb_clear(msl_kfdb *db) noexcept {
    try {
    return kfdb_clear(db);
    } MSL_ABI_CATCH_INT
}

int msl_kfdb_size(msl_kfdb *db, int32_t *n_slots, int32_t *n_live) noexcept {
    try {
    if (!db || !n_slots || !n_live) { set_error("msl_kfdb_size: null argument"); return MSL_ERR_INVALID; }
    std::lock_guard<std::mutex> lock(db->mutex);
    *n_slots = (int32_t)db->hostLive.size(); *n_live = db->nLive;
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}

int msl_reloc_candidates(msl_match *h, msl_kfdb *db, const msl_vocab *voc, int n_frames, int cap, int ccap, const int32_t *bow_word,
                         const double *bow_value, const int32_t *n_words, const int32_t *covis, msl_mem mem, int32_t *cand_out, int32_t *n_cand,
                         int32_t *words_out, float *score_out, msl_mem out_mem) noexcept {
    try {
    return handle_form(WHO_RELOC, check_reloc, launch_reloc, h, db, voc, n_frames, cap, ccap, bow_word, bow_value, n_words, covis, mem, cand_out, n_cand,
                       words_out, score_out, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_reloc_candidates_batch(int device, msl_kfdb *db, const msl_vocab *voc, int n_frames, int cap, int ccap, const int32_t *bow_word,
                               const double *bow_value, const int32_t *n_words, const int32_t *covis, msl_mem mem, int32_t *cand_out,
                               int32_t *n_cand, int32_t *words_out, float *score_out, msl_mem out_mem) noexcept {
    try {
    return batch_form(check_reloc, launch_reloc, device, mem == MSL_MEM_DEVICE, db, voc, n_frames, cap, ccap, bow_word, bow_value, n_words, covis, mem,
                      cand_out, n_cand, words_out, score_out, out_mem);
    } MSL_ABI_CATCH_INT
}

}  // extern "C"

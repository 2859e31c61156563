// msl_fuse.hip -- the point half of LocalMapping::SearchInNeighbors for gfx950 (reference src/LocalMapping.cc:545-569): ORBmatcher::Fuse
// (src/ORBmatcher.cc:408-546) with KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:469-504) and MapPoint::PredictScale (src/MapPoint.cc:350-364)
// as msl_fuse_map_points[_batch], the de-duplicated candidate list of :553-567 as msl_fuse_candidates[_batch].
//
// The search of one (target keyframe, map point) pair reads the keyframe's features and pose and the point's own position, normal,
// distance range and descriptor, never a slot and never another candidate; only the add / replace choice is ordered.  So every (item,
// candidate) is searched from the state on entry and the choice is resolved from that state too, as far as it is known (msl.h):
//   k_match_grid    (msl_match_window.h) one workgroup per TABLE keyframe: the 64 x 48 grid as a cell-sorted item list
//   k_fuse_held     one workgroup per table keyframe: the ids its slots hold, sorted in LDS -> IsInKeyFrame is a binary search
//   k_fuse_search   one wave per (item, candidate): the exits of the loop body in order, wave-uniform, each a few instructions; then the
//                   window's cells over the lanes, the filters, popcount distance; wave minimum of (dist << 16 | item position) = the first
//                   minimum in walk order, because item positions ascend in it
//   k_fuse_resolve  one workgroup per item: the first and the second matched j of every slot by two LDS atomicMin passes.  The slot walk of
//                   msl.h has a closed form on them: the first hit resolves from the entry state, the second only after an ADDED (whose
//                   nobs is known), every later one is UNRESOLVED (HELD_BAD stays HELD_BAD); `other` follows the holder.  n_fused by a
//                   block count
//   k_fuse_cand     one workgroup per item: position = target rank * cap + slot; the smallest position of every id by atomicMin into the
//                   item's row of scratch (only the ids met are reset first, so no pass is as long as the point table), the positions that
//                   won, an ordered compaction by prefix count
// Pins (tests/fuse_model.py is the sequential model; contraction off): the arithmetic of msl.h's "reproduced exactly" list; a keypoint
// octave outside [0, nlevels) is never a candidate; a held_id outside [0, n_pts) is an empty slot; device-only: an id outside the point
// table is NULL, a tgt outside the keyframe table has no pose, so its live candidates leave as NO_FEATURE, a list outside the lists is empty.
#include "msl_fuse_list.h"
#include "msl_index_check.h"
#include "msl_match_window.h"

#include <algorithm>

namespace {

using namespace msl;

constexpr int MAX_TCAP = 64;
constexpr int HELD_NT = 1024, SEARCH_NT = 256, RESOLVE_NT = 1024, CAND_NT = 1024;
constexpr size_t CAND_SCRATCH = (size_t)1 << 24;   // entries of msl_fuse_candidates' scratch: the items in flight share it

// What msl_debug_fuse reads per (item, candidate)
struct FuseRec { float u, v, ur; int32_t level, nidx; };

struct FuseDev {
    int nTab, cap, nPts, nItems, nLists, lcap, P;
    msl_fuse_params prm;
    MatchDev G;                                    // the grid of the table keyframes (pair = table index)
    const msl_keypoint *kps; const float *uright; const uint8_t *desc; const int32_t *n; const float *Tcw; const int32_t *held;
    const float *xyz, *normal, *dist; const uint8_t *pdesc, *flags; const int32_t *nobs;
    const int32_t *tgt, *list, *cand, *nCand;
    int32_t *bestIdx, *bestDist; uint8_t *status; int32_t *other, *nFused;
    unsigned *heldSorted; FuseRec *rec;
};

// ==== the ids every table keyframe holds, ascending ==========================================================================================
__global__ __launch_bounds__(HELD_NT) void k_fuse_held(FuseDev D) {
    extern __shared__ unsigned long long s_key[];
    const int k = blockIdx.x, P = D.P;
    const int n = clampi(D.n[k], 0, D.cap);
    for (int i = threadIdx.x; i < P; i += HELD_NT) {
        unsigned long long key = ~0ull;
        if (i < n) {
            const int id = D.held[(size_t)k * D.cap + i];
            if (id >= 0 && id < D.nPts) key = (unsigned long long)(unsigned)id;
        }
        s_key[i] = key;
    }
    bitonic_sort(s_key, P);
    for (int i = threadIdx.x; i < P; i += HELD_NT) D.heldSorted[(size_t)k * P + i] = s_key[i] == ~0ull ? NO_ENTRY : (unsigned)s_key[i];
}

// ==== the loop body of ORBmatcher::Fuse up to bestDist ========================================================================================
__global__ __launch_bounds__(SEARCH_NT) void k_fuse_search(FuseDev D) {
    const int f = blockIdx.y, lane = lane_id();
    const int j = blockIdx.x * (SEARCH_NT / WAVE) + (threadIdx.x >> 6);
    if (j >= D.lcap) return;                                                   // uniform per wave, as everything up to the window walk
    const size_t o = (size_t)f * D.lcap + j;
    const int32_t *row;
    const int nc = item_list(D, f, row);
    FuseRec R{};
    int status = MSL_FUSE_NULL, bestIdx = -1, bestDist = 0;
    if (j < nc) {
        bestDist = 256;
        const int id = row[j];
        const int k = D.tgt[f];
        const bool kf = k >= 0 && k < D.nTab;
        const msl_fuse_params &K = D.prm;
        do {
            if (id < 0 || id >= D.nPts) break;                                 // :427
            status = MSL_FUSE_BAD;
            if (!(D.flags[id] & 1)) break;                                     // :430 isBad()
            status = MSL_FUSE_NO_FEATURE;
            if (!kf) break;
            status = MSL_FUSE_IN_KEYFRAME;
            const unsigned *hs = D.heldSorted + (size_t)k * D.P;
            int lo = 0, hi = D.P;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (hs[mid] < (unsigned)id) lo = mid + 1; else hi = mid; }
            if (lo < D.P && hs[lo] == (unsigned)id) break;                     // :430 IsInKeyFrame(pKF)
            const float *T = D.Tcw + (size_t)k * 12;
            const float tcw[3] = {T[3], T[7], T[11]};
            const float p3Dw[3] = {D.xyz[3 * (size_t)id], D.xyz[3 * (size_t)id + 1], D.xyz[3 * (size_t)id + 2]};
            float p3Dc[3];
            gemm3(T, false, 1.0, p3Dw, tcw, p3Dc);                             // :434
            status = MSL_FUSE_BEHIND;
            if (p3Dc[2] < 0.0f) break;                                         // :437
            const float invz = (float)(1.0 / (double)p3Dc[2]);                 // the float division, correctly rounded
            const float x = p3Dc[0] * invz, y = p3Dc[1] * invz;
            const float u = K.fx * x + K.cx, v = K.fy * y + K.cy;
            R.u = u; R.v = v;
            status = MSL_FUSE_OUT_OF_IMAGE;
            if (!(u >= K.minX && u < K.maxX && v >= K.minY && v < K.maxY)) break;   // KeyFrame::IsInImage
            const float ur = u - K.bf * invz;
            R.ur = ur;
            const float maxDistance = 1.2f * D.dist[2 * (size_t)id + 1], minDistance = 0.8f * D.dist[2 * (size_t)id];
            float Ow[3];
            camera_centre(T, Ow);
            const float PO[3] = {p3Dw[0] - Ow[0], p3Dw[1] - Ow[1], p3Dw[2] - Ow[2]};
            double s2 = 0.0;                                                   // cv::norm(PO): norm3_dacc, written out (k_fuse_search's text)
#pragma unroll
            for (int a = 0; a < 3; a++) s2 += (double)PO[a] * (double)PO[a];
            const double dot = dot3_dacc(PO, D.normal + 3 * (size_t)id);
            const float dist3D = (float)sqrt(s2);
            status = MSL_FUSE_DISTANCE;
            if (dist3D < minDistance || dist3D > maxDistance) break;           // :459
            status = MSL_FUSE_VIEW_ANGLE;
            if (dot < 0.5 * (double)dist3D) break;                             // :465
            const int level = predict_scale(D.dist[2 * (size_t)id + 1], dist3D, K.log_scale_factor, K.nlevels);
            const float radius = K.th * K.scale_factors[level];
            R.level = level;
            // GetFeaturesInArea and the candidate loop, the window's cells over the lanes
            Query Q;
            unsigned key = KEY_NONE;
            int cnt = 0;
            if (grid_window(D.G, u, v, radius, Q)) {
                const size_t base = (size_t)k * D.cap;
                const unsigned short *items = D.G.items + base;
                uint4 d0, d1;
                load_desc(D.pdesc + (size_t)id * 32, d0, d1);
                const int C = window_cells(Q);
                for (int c = lane; c < C; c += WAVE) {
                    unsigned b, e;
                    window_cell(D.G, k, Q, c, b, e);
                    for (unsigned p = b; p < e; p++) {
                        const size_t i = base + items[p];
                        const msl_keypoint *kp = D.kps + i;
                        const float kpx = kp->x, kpy = kp->y;
                        if (!(fabsf(kpx - u) < radius && fabsf(kpy - v) < radius)) continue;
                        cnt++;
                        const int kpLevel = kp->octave;
                        if (kpLevel < level - 1 || kpLevel > level || kpLevel < 0 || kpLevel >= K.nlevels) continue;
                        const float kpr = D.uright[i];
                        const float ex = u - kpx, ey = v - kpy;
                        if (kpr >= 0) {
                            const float er = ur - kpr;
                            const float e2 = ex * ex + ey * ey + er * er;
                            if ((double)(e2 * K.inv_level_sigma2[kpLevel]) > 7.8) continue;
                        } else {
                            const float e2 = ex * ex + ey * ey;
                            if ((double)(e2 * K.inv_level_sigma2[kpLevel]) > 5.99) continue;
                        }
                        uint4 e0, e1;
                        load_desc(D.desc + i * 32, e0, e1);
                        const unsigned dist = (unsigned)hamming256(d0, d1, e0, e1);
                        if (dist < 256u) { const unsigned kk = (dist << 16) | p; key = kk < key ? kk : key; }
                    }
                }
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {                          // wave_min and wave_sum, one shuffle pair per offset
                const unsigned ok = (unsigned)__shfl_xor((int)key, off);
                key = ok < key ? ok : key;
                cnt += __shfl_xor(cnt, off);
            }
            R.nidx = cnt;
            status = MSL_FUSE_NO_FEATURE;
            if (cnt == 0) break;                                               // :475
            status = MSL_FUSE_NO_CANDIDATE;
            if (key == KEY_NONE) break;
            bestDist = (int)(key >> 16);
            bestIdx = D.G.items[(size_t)k * D.cap + (key & 0xFFFFu)];
            status = bestDist <= K.th_low ? MSL_FUSE_ADDED : MSL_FUSE_ABOVE_TH_LOW;   // ADDED: matched; k_fuse_resolve decides
        } while (false);
    }
    if (lane == 0) {
        D.bestIdx[o] = bestIdx; D.bestDist[o] = bestDist; D.status[o] = (uint8_t)status; D.other[o] = -1;
        D.rec[o] = R;
    }
}

// ==== the slot walk ==========================================================================================================================
__global__ __launch_bounds__(RESOLVE_NT) void k_fuse_resolve(FuseDev D) {
    extern __shared__ unsigned s_hit[];                                        // [cap] first, [cap] second matched j of every slot
    const int f = blockIdx.x, cap = D.cap;
    unsigned *first = s_hit, *second = s_hit + cap;
    const int32_t *row;
    const int nc = item_list(D, f, row);
    const int k = D.tgt[f];
    const size_t fb = (size_t)f * D.lcap;
    for (int s = threadIdx.x; s < 2 * cap; s += RESOLVE_NT) s_hit[s] = NO_ENTRY;
    __syncthreads();
    first_two_hits<RESOLVE_NT>(D.status, D.bestIdx, fb, MSL_FUSE_ADDED, nc, first, second, [](int, int) { return false; });
    int mine = 0;
    for (int j = threadIdx.x; j < nc; j += RESOLVE_NT) {
        if (D.status[fb + j] != MSL_FUSE_ADDED) continue;                      // a matched candidate: its tgt is a table keyframe
        mine++;
        const int s = D.bestIdx[fb + j];
        int h0 = D.held[(size_t)k * cap + s];
        if (h0 < 0 || h0 >= D.nPts) h0 = -1;
        const unsigned j1 = first[s], j2 = second[s];
        const int p1 = row[j1];
        int st, oth;
        if (h0 >= 0 && !(D.flags[h0] & 1)) { st = MSL_FUSE_HELD_BAD; oth = h0; }
        else if (h0 < 0) {
            if ((unsigned)j == j1) { st = MSL_FUSE_ADDED; oth = -1; }
            else {                                                             // the holder is p1 with the observation it just got
                const int p2 = row[j2];
                const bool keeps = D.nobs[p1] + (D.uright[(size_t)k * cap + s] >= 0 ? 2 : 1) > D.nobs[p2];
                if ((unsigned)j == j2) { st = keeps ? MSL_FUSE_REPLACED_BY_HELD : MSL_FUSE_REPLACES_HELD; oth = p1; }
                else { st = MSL_FUSE_UNRESOLVED; oth = keeps ? p1 : p2; }
            }
        } else {
            const bool keeps = D.nobs[h0] > D.nobs[p1];
            if ((unsigned)j == j1) { st = keeps ? MSL_FUSE_REPLACED_BY_HELD : MSL_FUSE_REPLACES_HELD; oth = h0; }
            else { st = MSL_FUSE_UNRESOLVED; oth = keeps ? h0 : p1; }
        }
        D.status[fb + j] = (uint8_t)st; D.other[fb + j] = oth;
    }
    mine = wave_sum(mine);
    __syncthreads();                                                           // the hits are read: s_hit[0] becomes the count
    if (threadIdx.x == 0) s_hit[0] = 0;
    __syncthreads();
    if (lane_id() == 0 && mine) atomicAdd(&s_hit[0], (unsigned)mine);
    __syncthreads();
    if (threadIdx.x == 0) D.nFused[f] = (int)s_hit[0];
}

// ==== vpFuseCandidates =======================================================================================================================
struct CandDev {
    int nTab, cap, nPts, tcap, lcap, item0;
    const int32_t *held, *n; const uint8_t *flags; const int32_t *targets, *nTargets;
    int32_t *cand, *nCand; unsigned *first;
};

// The live point id at position pos = target rank * cap + slot of item f, or -1
__device__ __forceinline__ int cand_id(const CandDev &D, int f, int pos) {
    const int t = pos / D.cap, i = pos - t * D.cap;
    const int k = D.targets[(size_t)f * D.tcap + t];
    if (k < 0 || k >= D.nTab || i >= D.n[k]) return -1;
    const int id = D.held[(size_t)k * D.cap + i];
    if (id < 0 || id >= D.nPts || !(D.flags[id] & 1)) return -1;
    return id;
}

__global__ __launch_bounds__(CAND_NT) void k_fuse_cand(CandDev D) {
    __shared__ unsigned s_wave[CAND_NT / WAVE];
    const int f = D.item0 + blockIdx.x, lane = lane_id(), w = threadIdx.x >> 6;
    unsigned *first = D.first + (size_t)blockIdx.x * D.nPts;                    // this workgroup's row; read and written with atomics only
    const int total = clampi(D.nTargets[f], 0, D.tcap) * D.cap;
    for (int pos = threadIdx.x; pos < total; pos += CAND_NT) {
        const int id = cand_id(D, f, pos);
        if (id >= 0) __hip_atomic_store(&first[id], NO_ENTRY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __threadfence(); __syncthreads();
    for (int pos = threadIdx.x; pos < total; pos += CAND_NT) {
        const int id = cand_id(D, f, pos);
        if (id >= 0) atomicMin(&first[id], (unsigned)pos);
    }
    __threadfence(); __syncthreads();
    int32_t *out = D.cand + (size_t)f * D.lcap;
    int kept = 0;                                                              // uniform: the candidates before this chunk
    for (int at = 0; at < total; at += CAND_NT) {
        const int pos = at + threadIdx.x;
        const int id = pos < total ? cand_id(D, f, pos) : -1;
        const bool keep = id >= 0 && __hip_atomic_load(&first[id], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)pos;
        const unsigned long long m = __ballot(keep);
        if (lane == 0) s_wave[w] = (unsigned)__popcll(m);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int q = 0; q < CAND_NT / WAVE; q++) { const int c = (int)s_wave[q]; all += c; before += q < w ? c : 0; }
        if (keep) {
            const int rank = kept + before + __popcll(m & ((1ull << lane) - 1ull));
            if (rank < D.lcap) out[rank] = id;
        }
        kept += all;
        __syncthreads();
    }
    for (int q = kept + threadIdx.x; q < D.lcap; q += CAND_NT) out[q] = -1;
    if (threadIdx.x == 0) D.nCand[f] = kept;
}

// ==== host side ==============================================================================================================================
const char *const WHO_CAND = "msl_fuse_candidates", *const WHO_FUSE = "msl_fuse_map_points";

int check_fuse_candidates(int n_tab, int cap, int n_pts, int n_items, int tcap, int lcap, const int32_t *held_id, const int32_t *n_kps,
                          const uint8_t *pt_flags, const int32_t *targets, const int32_t *n_targets, msl_mem mem, int32_t *cand, int32_t *n_cand,
                          msl_mem) {
    const char *who = WHO_CAND;
    if (!none_null(who, {MSL_NAMED(held_id), MSL_NAMED(n_kps), MSL_NAMED(pt_flags), MSL_NAMED(targets), MSL_NAMED(n_targets), MSL_NAMED(cand),
                         MSL_NAMED(n_cand)})) return MSL_ERR_INVALID;
    if (!table_limits(who, n_tab, cap, n_pts) || !item_limits(who, n_items, lcap)) return MSL_ERR_INVALID;
    if (tcap < 1 || tcap > MAX_TCAP) { set_error("%s: tcap %d outside 1 .. %d", who, tcap, MAX_TCAP); return MSL_ERR_INVALID; }
    char why[256];
    if (mem == MSL_MEM_HOST && !check::targets_ok(n_tab, n_items, tcap, targets, n_targets, why, sizeof(why))) return refuse(who, why);
    return MSL_OK;
}

int launch_fuse_candidates(msl_match *h, int n_tab, int cap, int n_pts, int n_items, int tcap, int lcap, const int32_t *held_id,
                           const int32_t *n_kps, const uint8_t *pt_flags, const int32_t *targets, const int32_t *n_targets, msl_mem mem,
                           int32_t *cand, int32_t *n_cand, msl_mem out_mem) {
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    hipStream_t st = h->stream;
    // the items in flight at once: each has a row of n_pts entries in the scratch
    const int flight = (int)std::min<size_t>((size_t)n_items, std::max<size_t>(1, CAND_SCRATCH / (size_t)n_pts));
    MSL_HIP_TRY(grow_all(st, {{h->fuseFirst, (size_t)flight * n_pts * sizeof(unsigned)}}));
    const size_t T = (size_t)n_tab, F = (size_t)n_items;
    CandDev D{};
    D.nTab = n_tab; D.cap = cap; D.nPts = n_pts; D.tcap = tcap; D.lcap = lcap;
    Stage S(h, mem, out_mem);
    D.held = S.in(held_id, T * cap); D.n = S.in(n_kps, T); D.flags = S.in(pt_flags, (size_t)n_pts); D.targets = S.in(targets, F * tcap);
    D.nTargets = S.in(n_targets, F);
    D.cand = S.out(cand, F * lcap); D.nCand = S.out(n_cand, F);
    D.first = (unsigned *)h->fuseFirst.p;
    MSL_HIP_TRY(S.error());
    for (int f0 = 0; f0 < n_items; f0 += flight) {                             // stream order keeps the chunks off each other's rows
        D.item0 = f0;
        hipLaunchKernelGGL(k_fuse_cand, dim3((unsigned)std::min(flight, n_items - f0)), dim3(CAND_NT), 0, st, D);
        MSL_HIP_TRY(hipGetLastError());
    }
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}

int check_fuse(int n_tab, int cap, int n_pts, int n_items, int n_lists, int lcap, const msl_fuse_params *params, const msl_keypoint *kps_un,
               const float *uright, const int32_t *grid_cell, const uint8_t *desc, const int32_t *n_kps, const float *Tcw, const int32_t *held_id,
               const float *pt_xyz, const float *pt_normal, const float *pt_dist, const uint8_t *pt_desc, const uint8_t *pt_flags,
               const int32_t *pt_nobs, const int32_t *tgt, const int32_t *list, const int32_t *cand, const int32_t *n_cand, msl_mem mem,
               int32_t *best_idx, int32_t *best_dist, uint8_t *status, int32_t *other, int32_t *n_fused, msl_mem) {
    const char *who = WHO_FUSE;
    if (!none_null(who, {MSL_NAMED(params), MSL_NAMED(kps_un), MSL_NAMED(uright), MSL_NAMED(grid_cell), MSL_NAMED(desc), MSL_NAMED(n_kps),
                         MSL_NAMED(Tcw), MSL_NAMED(held_id), MSL_NAMED(pt_xyz), MSL_NAMED(pt_normal), MSL_NAMED(pt_dist), MSL_NAMED(pt_desc),
                         MSL_NAMED(pt_flags), MSL_NAMED(pt_nobs), MSL_NAMED(tgt), MSL_NAMED(list), MSL_NAMED(cand), MSL_NAMED(n_cand),
                         MSL_NAMED(best_idx), MSL_NAMED(best_dist), MSL_NAMED(status), MSL_NAMED(other), MSL_NAMED(n_fused)})) return MSL_ERR_INVALID;
    if (!table_limits(who, n_tab, cap, n_pts) || !item_limits(who, n_items, lcap)) return MSL_ERR_INVALID;
    if (n_lists < 1) { set_error("%s: n_lists %d below 1", who, n_lists); return MSL_ERR_INVALID; }
    if (!levels_ok(who, params->nlevels)) return MSL_ERR_INVALID;
    if (params->th_low < 0 || params->th_low > 255) { set_error("%s: th_low %d outside 0 .. 255", who, params->th_low); return MSL_ERR_INVALID; }
    char why[256];
    if (mem == MSL_MEM_HOST && !check::lists_ok("point", n_tab, n_pts, n_items, n_lists, lcap, tgt, list, cand, n_cand, why, sizeof(why))) return refuse(who, why);
    return MSL_OK;
}

int launch_fuse(msl_match *h, int n_tab, int cap, int n_pts, int n_items, int n_lists, int lcap, const msl_fuse_params *prm,
                const msl_keypoint *kps_un, const float *uright, const int32_t *grid_cell, const uint8_t *desc, const int32_t *n_kps, const float *Tcw,
                const int32_t *held_id, const float *pt_xyz, const float *pt_normal, const float *pt_dist, const uint8_t *pt_desc,
                const uint8_t *pt_flags, const int32_t *pt_nobs, const int32_t *tgt, const int32_t *list, const int32_t *cand, const int32_t *n_cand,
                msl_mem mem, int32_t *best_idx, int32_t *best_dist, uint8_t *status, int32_t *other, int32_t *n_fused, msl_mem out_mem) {
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    hipStream_t st = h->stream;
    const size_t T = (size_t)n_tab, nt = T * cap, F = (size_t)n_items, L = (size_t)n_lists, np = (size_t)n_pts, nf = F * lcap;
    FuseDev D{};
    D.nTab = n_tab; D.cap = cap; D.nPts = n_pts; D.nItems = n_items; D.nLists = n_lists; D.lcap = lcap; D.P = pow2_at_least(cap > 2 ? cap : 2);
    D.prm = *prm;
    MSL_HIP_TRY(grow_all(st, {{h->items, sizeof(unsigned short) * nt}, {h->cellStart, sizeof(unsigned) * (NCELLS + 1) * T},
                              {h->fuseHeld, sizeof(unsigned) * T * D.P}, {h->fuseRec, sizeof(FuseRec) * nf}}));
    h->fuseItems = n_items; h->fuseLcap = lcap;
    Stage S(h, mem, out_mem);
    D.kps = S.in(kps_un, nt); D.uright = S.in(uright, nt);
    const int32_t *cell = S.in(grid_cell, nt);
    D.desc = S.in(desc, 32 * nt); D.n = S.in(n_kps, T); D.Tcw = S.in(Tcw, 12 * T); D.held = S.in(held_id, nt);
    D.xyz = S.in(pt_xyz, 3 * np); D.normal = S.in(pt_normal, 3 * np); D.dist = S.in(pt_dist, 2 * np); D.pdesc = S.in(pt_desc, 32 * np);
    D.flags = S.in(pt_flags, np); D.nobs = S.in(pt_nobs, np);
    D.tgt = S.in(tgt, F); D.list = S.in(list, F); D.cand = S.in(cand, L * lcap); D.nCand = S.in(n_cand, L);
    D.bestIdx = S.out(best_idx, nf); D.bestDist = S.out(best_dist, nf); D.status = S.out(status, nf); D.other = S.out(other, nf);
    D.nFused = S.out(n_fused, F);
    MSL_HIP_TRY(S.error());
    D.heldSorted = (unsigned *)h->fuseHeld.p; D.rec = (FuseRec *)h->fuseRec.p;
    // the grid of every table keyframe: what k_match_grid and the window helpers read of a MatchDev
    MatchDev &G = D.G;
    G.nPairs = n_tab; G.cap = cap;
    G.prm.minX = prm->minX; G.prm.maxX = prm->maxX; G.prm.minY = prm->minY; G.prm.maxY = prm->maxY;
    G.gridWInv = static_cast<float>(GRID_COLS) / static_cast<float>(prm->maxX - prm->minX);   // src/Frame.cc:137-138, copied by the KeyFrame
    G.gridHInv = static_cast<float>(GRID_ROWS) / static_cast<float>(prm->maxY - prm->minY);
    G.curCell = cell; G.nCur = D.n;
    G.items = (unsigned short *)h->items.p; G.cellStart = (unsigned *)h->cellStart.p; G.mode = nullptr;
    MSL_HIP_TRY(allow_lds(h, LDS_FUSE_HELD, k_fuse_held, 8 * MAX_CAP));
    MSL_HIP_TRY(allow_lds(h, LDS_FUSE_RESOLVE, k_fuse_resolve, 8 * MAX_CAP));
    hipLaunchKernelGGL(k_match_grid, dim3((unsigned)n_tab), dim3(256), sizeof(unsigned short) * cap, st, G);
    MSL_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_fuse_held, dim3((unsigned)n_tab), dim3(HELD_NT), 8 * (size_t)D.P, st, D);
    MSL_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_fuse_search, dim3((unsigned)((lcap + SEARCH_NT / WAVE - 1) / (SEARCH_NT / WAVE)), (unsigned)n_items), dim3(SEARCH_NT), 0, st, D);
    MSL_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_fuse_resolve, dim3((unsigned)n_items), dim3(RESOLVE_NT), 8 * (size_t)cap, st, D);
    MSL_HIP_TRY(hipGetLastError());
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}

}  // namespace

extern "C" {

int msl_fuse_candidates(msl_match *h, int n_tab, int cap, int n_pts, int n_items, int tcap, int lcap, const int32_t *held_id, const int32_t *n_kps,
                        const uint8_t *pt_flags, const int32_t *targets, const int32_t *n_targets, msl_mem mem, int32_t *cand, int32_t *n_cand,
                        msl_mem out_mem) noexcept {
    try {
    return handle_form(WHO_CAND, check_fuse_candidates, launch_fuse_candidates, h, n_tab, cap, n_pts, n_items, tcap, lcap, held_id, n_kps, pt_flags,
                       targets, n_targets, mem, cand, n_cand, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_fuse_candidates_batch(int device, int n_tab, int cap, int n_pts, int n_items, int tcap, int lcap, const int32_t *held_id,
                              const int32_t *n_kps, const uint8_t *pt_flags, const int32_t *targets, const int32_t *n_targets, msl_mem mem,
                              int32_t *cand, int32_t *n_cand, msl_mem out_mem) noexcept {
    try {
    return batch_form(check_fuse_candidates, launch_fuse_candidates, device, mem == MSL_MEM_DEVICE, n_tab, cap, n_pts, n_items, tcap, lcap, held_id,
                      n_kps, pt_flags, targets, n_targets, mem, cand, n_cand, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_fuse_map_points(msl_match *h, int n_tab, int cap, int n_pts, int n_items, int n_lists, int lcap, const msl_fuse_params *params,
                        const msl_keypoint *kps_un, const float *uright, const int32_t *grid_cell, const uint8_t *desc, const int32_t *n_kps,
                        const float *Tcw, const int32_t *held_id, const float *pt_xyz, const float *pt_normal, const float *pt_dist,
                        const uint8_t *pt_desc, const uint8_t *pt_flags, const int32_t *pt_nobs, const int32_t *tgt, const int32_t *list,
                        const int32_t *cand, const int32_t *n_cand, msl_mem mem, int32_t *best_idx, int32_t *best_dist, uint8_t *status,
                        int32_t *other, int32_t *n_fused, msl_mem out_mem) noexcept {
    try {
    return handle_form(WHO_FUSE, check_fuse, launch_fuse, h, n_tab, cap, n_pts, n_items, n_lists, lcap, params, kps_un, uright, grid_cell, desc, n_kps,
                       Tcw, held_id, pt_xyz, pt_normal, pt_dist, pt_desc, pt_flags, pt_nobs, tgt, list, cand, n_cand, mem, best_idx, best_dist, status,
                       other, n_fused, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_fuse_map_points_batch(int device, int n_tab, int cap, int n_pts, int n_items, int n_lists, int lcap, const msl_fuse_params *params,
                              const msl_keypoint *kps_un, const float *uright, const int32_t *grid_cell, const uint8_t *desc, const int32_t *n_kps,
                              const float *Tcw, const int32_t *held_id, const float *pt_xyz, const float *pt_normal, const float *pt_dist,
                              const uint8_t *pt_desc, const uint8_t *pt_flags, const int32_t *pt_nobs, const int32_t *tgt, const int32_t *list,
                              const int32_t *cand, const int32_t *n_cand, msl_mem mem, int32_t *best_idx, int32_t *best_dist, uint8_t *status,
                              int32_t *other, int32_t *n_fused, msl_mem out_mem) noexcept {
    try {
    return batch_form(check_fuse, launch_fuse, device, mem == MSL_MEM_DEVICE, n_tab, cap, n_pts, n_items, n_lists, lcap, params, kps_un, uright,
                      grid_cell, desc, n_kps, Tcw, held_id, pt_xyz, pt_normal, pt_dist, pt_desc, pt_flags, pt_nobs, tgt, list, cand, n_cand, mem, best_idx,
                      best_dist, status, other, n_fused, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_debug_fuse(msl_match *h, int item, float *uvr, int32_t *level_n) noexcept {
    try {
    if (!h || !uvr || !level_n || item < 0 || item >= h->fuseItems || !h->fuseRec.p) {
        set_error("msl_debug_fuse: invalid argument (item outside the last msl_fuse_map_points call?)");
        return MSL_ERR_INVALID;
    }
    std::vector<FuseRec> rec;
    int rc = last_call_row(h, h->fuseRec, (size_t)item, (size_t)h->fuseLcap, rec);
    if (rc != MSL_OK) return rc;
    for (int j = 0; j < h->fuseLcap; j++) {
        const FuseRec &r = rec[(size_t)j];
        uvr[3 * j] = r.u; uvr[3 * j + 1] = r.v; uvr[3 * j + 2] = r.ur;
        level_n[2 * j] = r.level; level_n[2 * j + 1] = r.nidx;
    }
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}

}  // extern "C"

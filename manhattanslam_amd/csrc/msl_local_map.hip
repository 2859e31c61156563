// msl_local_map.hip -- the first step of Tracking::TrackLocalMap for gfx950: Tracking::UpdateLocalKeyFrames (reference src/Tracking.cc:1813-1907)
// as msl_local_keyframes[_batch]; UpdateLocalPoints (:1789-1810) and UpdateLocalLines (:1766-1787), each fused with the first loop of
// SearchLocalPoints (:1656-1668) / SearchLocalLines (:1698-1710) and the gather out of the point / line table, as msl_local_points[_batch] and
// msl_local_lines[_batch].  What they write is what msl_match_local_points / msl_match_local_lines read.
//   k_local_kf   one workgroup of 1024 per frame.  The votes are integer LDS counters (one atomicAdd per observation of a live held point: exact
//                whatever the arrival order); the parent links and a state byte per keyframe (live, in the list) sit in LDS beside them.
//                Wave 0 then runs the two loops: the first as a ballot compaction in ascending table index, the second sequentially over at
//                most 80 keyframes, each search (first eligible neighbour of ten, first eligible child) a ballot and a find-first-set
//   k_lm_stamp   one workgroup per (frame, list position): atomicMin of (position * cap + slot) << 1 | 1 into the frame's stamp of every live
//                id the keyframe holds -- the first occurrence in list order wins whatever the arrival order
//   k_lm_held    the frame's own slots: cur_flags, and bit 0 of the stamp cleared for every live id the frame holds
//   k_lm_count   per (frame, list position) the slots whose key is the stamp;  k_lm_scan  their exclusive scan over the list, n_local
//   k_lm_write   per (frame, list position) a block scan over the slots gives every kept slot its place: the id, the rows, the flags
// The stamps are all ones before k_lm_stamp; frames run in groups whose stamps stay under the handle's budget.
// Pins (tests/localmap_model.py is the sequential model): msl.h's list; device-only: an index outside its table is absent.
#include "msl_match_handle.h"
#include "msl_index_check.h"
#include "msl_obs_walk.h"

#include <type_traits>

namespace {

using namespace msl;

constexpr int LM_NT = 256, LKF_NT = 1024, LOCAL_KF_STOP = 80, BEST_COVIS = 10, MAX_GROUP = 32768;
static_assert(MAX_TAB <= 4096 && MAX_CAP <= 8192, "a stamp key (position * cap + slot) << 1 | 1 fits 32 bits, a table index 15");

__device__ __forceinline__ unsigned wave_max(unsigned v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { const unsigned o = (unsigned)__shfl_xor((int)v, off); v = o > v ? o : v; }
    return v;
}

// ==== UpdateLocalKeyFrames of one frame ======================================================================================================
struct LocalKfDev {
    int cap, nTab, nPts, nObs, ccap;
    const int32_t *held, *nCur; const uint8_t *flags; const int32_t *off, *okf; const uint8_t *kfFlags;
    const int32_t *conn, *nConn, *parent, *prev, *nPrev;
    int32_t *votes, *list, *nList, *ref; uint8_t *cleared, *status;
};

__global__ __launch_bounds__(LKF_NT) void k_local_kf(LocalKfDev D) {
    __shared__ unsigned s_cnt[MAX_TAB];                                        // keyframeCounter
    __shared__ int16_t s_parent[MAX_TAB];                                      // mpParent as a table index, -1 for none
    __shared__ uint16_t s_list[MAX_TAB];                                       // mvpLocalKeyFrames
    __shared__ uint8_t s_state[MAX_TAB];                                       // bit 0: !isBad(), bit 1: mnTrackReferenceForFrame == F.mnId
    const int f = blockIdx.x, lane = threadIdx.x & (WAVE - 1);
    for (int j = threadIdx.x; j < D.nTab; j += LKF_NT) {
        const int p = D.parent[j];
        s_cnt[j] = 0; s_state[j] = D.kfFlags[j] & 1; s_parent[j] = (int16_t)(p >= 0 && p < D.nTab ? p : -1);
    }
    __syncthreads();
    const int nCur = clampi(D.nCur[f], 0, D.cap);
    for (int i = threadIdx.x; i < D.cap; i += LKF_NT) {
        const int id = i < nCur ? D.held[(size_t)f * D.cap + i] : -1;
        const bool known = id >= 0 && id < D.nPts, live = known && (D.flags[id] & 1);
        D.cleared[(size_t)f * D.cap + i] = known && !live;                     // :1825
        if (!live) continue;
        int b, e;
        obs_range(D, id, b, e);
        for (int o = b; o < e; o++) {
            const int k = D.okf[o];
            if (k >= 0 && k < D.nTab) atomicAdd(&s_cnt[k], 1u);                // a bad keyframe counts here and is filtered below
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < D.nTab; j += LKF_NT) D.votes[(size_t)f * D.nTab + j] = (int)s_cnt[j];
    if (threadIdx.x >= WAVE) return;                                           // the two loops are wave 0's: LDS in program order, no barrier
    volatile uint16_t *list = s_list;
    volatile uint8_t *state = s_state;
    int32_t *out = D.list + (size_t)f * D.nTab;
    const unsigned long long below = (1ull << lane) - 1ull;
    // the first loop: ascending table index, bad keyframes skipped, max by strict >
    int n = 0, bj = 0;
    unsigned bw = 0;
    bool any = false;
    for (int c = 0; c < D.nTab; c += WAVE) {
        const int j = c + lane;
        const unsigned w = j < D.nTab ? s_cnt[j] : 0u;
        any |= w > 0;
        const bool push = w > 0 && (state[j] & 1);
        const unsigned long long m = __ballot(push);
        if (push) {
            list[n + __popcll(m & below)] = (uint16_t)j; state[j] = 3;
            if (w > bw) { bw = w; bj = j; }
        }
        n += __popcll(m);
    }
    if (!__ballot(any)) {                                                      // keyframeCounter.empty(): the list stays as it was (:1830)
        const int np = D.prev ? clampi(D.nPrev[f], 0, D.nTab) : 0;
        for (int r = lane; r < D.nTab; r += WAVE) out[r] = r < np ? D.prev[(size_t)f * D.nTab + r] : -1;
        if (lane == 0) { D.nList[f] = np; D.ref[f] = -1; D.status[f] = MSL_LOCALMAP_NO_VOTES; }
        return;
    }
    const unsigned wmax = wave_max(bw);
    const int ref = wmax ? (int)wave_min(bw == wmax ? (unsigned)bj : ~0u) : -1;   // the lowest index among equal maxima
    // the second loop: over the entries of the first (the end iterator is taken before it)
    const int n1 = n;
    for (int it = 0; it < n1; it++) {
        if (n > LOCAL_KF_STOP) break;
        const int k = list[it];
        int nn = clampi(D.nConn[k], 0, D.ccap);
        nn = nn < BEST_COVIS ? nn : BEST_COVIS;
        const int c = lane < nn ? D.conn[(size_t)k * D.ccap + lane] : -1;
        unsigned long long m = __ballot(c >= 0 && c < D.nTab && state[c < 0 || c >= D.nTab ? 0 : c] == 1);   // live, not in the list
        if (m) {
            const int c0 = __shfl(c, __ffsll(m) - 1);
            if (lane == 0) { list[n] = (uint16_t)c0; state[c0] = 3; }
            n++;
        }
        for (int cc = 0; cc < D.nTab; cc += WAVE) {                            // spChilds in ascending table index
            const int j = cc + lane;
            m = __ballot(j < D.nTab && s_parent[j < D.nTab ? j : 0] == k && state[j < D.nTab ? j : 0] == 1);
            if (!m) continue;
            const int j0 = cc + __ffsll(m) - 1;
            if (lane == 0) { list[n] = (uint16_t)j0; state[j0] = 3; }
            n++;
            break;
        }
        const int p = s_parent[k];
        if (p >= 0 && !(state[p] & 2)) {                                       // no isBad test, and the break leaves the whole walk (:1897)
            if (lane == 0) { list[n] = (uint16_t)p; state[p] = state[p] | 2; }
            n++;
            break;
        }
    }
    for (int r = lane; r < D.nTab; r += WAVE) out[r] = r < n ? (int)list[r] : -1;
    if (lane == 0) { D.nList[f] = n; D.ref[f] = ref; D.status[f] = 0; }
}

// ==== UpdateLocalPoints / UpdateLocalLines: the ordered first-occurrence compaction ============================================================
// Everything but the rows: kcap slots per table keyframe, fcap per frame, nIds rows in the element table, mcap outputs per frame; frames
// f0 .. f0 + gridDim.y - 1 of the call are in flight, frame f0 + g on stamp row g.
struct LocalMapDev {
    int nTab, kcap, fcap, nIds, mcap, f0;
    const int32_t *list, *nList, *held, *nKf, *cur, *nCur;
    const uint8_t *flags; const int32_t *nobs;
    unsigned *stamp; int32_t *count;
    int32_t *outId, *nOut; uint8_t *outFlags, *curFlags;
};
// The rows of the element table and of the output, as words: W = uint32_t for float rows, uint64_t for double rows; NX words of position
template <class W>
struct LocalRows {
    const W *xyz, *normal; const uint32_t *dist; const uint8_t *desc;
    W *oXyz, *oNormal; uint32_t *oDist; uint8_t *oDesc;
};

// The keyframe at list position blockIdx.x of frame f0 + blockIdx.y and its slot count; false when there is none (beyond the list, or an
// index outside the table: absent)
__device__ __forceinline__ bool list_entry(const LocalMapDev &D, int &f, int &k, int &n) {
    f = D.f0 + (int)blockIdx.y;
    const int pos = blockIdx.x;
    k = -1; n = 0;
    if (pos >= clampi(D.nList[f], 0, D.nTab)) return false;
    k = D.list[(size_t)f * D.nTab + pos];
    if (k < 0 || k >= D.nTab) return false;
    n = clampi(D.nKf[k], 0, D.kcap);
    return true;
}
// The live id in slot i of keyframe k, or -1
__device__ __forceinline__ int live_id(const LocalMapDev &D, int k, int i) {
    const int id = D.held[(size_t)k * D.kcap + i];
    return id >= 0 && id < D.nIds && (D.flags[id] & 1) ? id : -1;
}
__device__ __forceinline__ unsigned stamp_key(const LocalMapDev &D, int i) { return (((unsigned)blockIdx.x * (unsigned)D.kcap + (unsigned)i) << 1) | 1u; }

__global__ __launch_bounds__(LM_NT) void k_lm_stamp(LocalMapDev D) {
    int f, k, n;
    if (!list_entry(D, f, k, n)) return;
    unsigned *stamp = D.stamp + (size_t)blockIdx.y * D.nIds;
    for (int i = threadIdx.x; i < n; i += LM_NT) {
        const int id = live_id(D, k, i);
        if (id >= 0) atomicMin(&stamp[id], stamp_key(D, i));
    }
}

__global__ __launch_bounds__(LM_NT) void k_lm_held(LocalMapDev D) {
    const int f = D.f0 + (int)blockIdx.y, i = blockIdx.x * LM_NT + threadIdx.x;
    if (i >= D.fcap) return;
    const int id = i < clampi(D.nCur[f], 0, D.fcap) ? D.cur[(size_t)f * D.fcap + i] : -1;
    const bool live = id >= 0 && id < D.nIds && (D.flags[id] & 1);
    D.curFlags[(size_t)f * D.fcap + i] = live ? (uint8_t)(1 | (D.nobs[id] > 0 ? 2 : 0)) : (uint8_t)0;
    if (live) atomicAnd(&D.stamp[(size_t)blockIdx.y * D.nIds + id], ~1u);     // mnLastFrameSeen = F.mnId (:1664)
}

__global__ __launch_bounds__(LM_NT) void k_lm_count(LocalMapDev D) {
    __shared__ int s_total;
    int f, k, n;
    const bool has = list_entry(D, f, k, n);
    if ((int)blockIdx.x >= clampi(D.nList[f], 0, D.nTab)) return;              // k_lm_scan reads the list's positions alone
    if (threadIdx.x == 0) s_total = 0;
    __syncthreads();
    const unsigned *stamp = D.stamp + (size_t)blockIdx.y * D.nIds;
    int cnt = 0;
    if (has)
        for (int i = threadIdx.x; i < n; i += LM_NT) {
            const int id = live_id(D, k, i);
            cnt += id >= 0 && (stamp[id] | 1u) == stamp_key(D, i) ? 1 : 0;
        }
    cnt = wave_sum(cnt);
    if ((threadIdx.x & (WAVE - 1)) == 0 && cnt) atomicAdd(&s_total, cnt);
    __syncthreads();
    if (threadIdx.x == 0) D.count[(size_t)blockIdx.y * D.nTab + blockIdx.x] = s_total;
}

__global__ __launch_bounds__(LM_NT) void k_lm_scan(LocalMapDev D) {
    __shared__ int s_arr[MAX_TAB];
    __shared__ unsigned s_wave[17];
    const int g = blockIdx.x, f = D.f0 + g, nl = clampi(D.nList[f], 0, D.nTab);
    int32_t *count = D.count + (size_t)g * D.nTab;
    for (int j = threadIdx.x; j < nl; j += LM_NT) s_arr[j] = count[j];
    __syncthreads();
    if (nl > 0) block_scan_array_incl(s_arr, nl, s_wave);
    for (int j = threadIdx.x; j < nl; j += LM_NT) count[j] = j ? s_arr[j - 1] : 0;
    const int total = nl > 0 ? s_arr[nl - 1] : 0;
    if (threadIdx.x == 0) D.nOut[f] = total;
    for (int j = (total < D.mcap ? total : D.mcap) + threadIdx.x; j < D.mcap; j += LM_NT) {
        D.outId[(size_t)f * D.mcap + j] = -1; D.outFlags[(size_t)f * D.mcap + j] = 0;
    }
}

template <class W, int NX>
__global__ __launch_bounds__(LM_NT) void k_lm_write(LocalMapDev D, LocalRows<W> R) {
    __shared__ unsigned s_wave[17];
    int f, k, n;
    if (!list_entry(D, f, k, n)) return;
    const unsigned *stamp = D.stamp + (size_t)blockIdx.y * D.nIds;
    int base = D.count[(size_t)blockIdx.y * D.nTab + blockIdx.x];
    for (int c = 0; c < n && base < D.mcap; c += LM_NT) {                      // uniform: every thread meets block_excl_scan's barriers
        const int i = c + threadIdx.x, id = i < n ? live_id(D, k, i) : -1;
        const unsigned st = id >= 0 ? stamp[id] : 0u;
        const bool kept = id >= 0 && (st | 1u) == stamp_key(D, i);
        unsigned total;
        const int j = base + (int)block_excl_scan(kept ? 1u : 0u, s_wave, &total);
        base += (int)total;
        if (!kept || j >= D.mcap) continue;
        const size_t o = (size_t)f * D.mcap + j, s = (size_t)id;
        D.outId[o] = id;
        D.outFlags[o] = (uint8_t)((st & 1u) | (D.nobs[id] > 0 ? 2u : 0u));    // bit 0: not among the frame's live held ids
#pragma unroll
        for (int a = 0; a < NX; a++) R.oXyz[NX * o + a] = R.xyz[NX * s + a];
#pragma unroll
        for (int a = 0; a < 3; a++) R.oNormal[3 * o + a] = R.normal[3 * s + a];
#pragma unroll
        for (int a = 0; a < 2; a++) R.oDist[2 * o + a] = R.dist[2 * s + a];
        const uint4 *d = reinterpret_cast<const uint4 *>(R.desc + 32 * s);
        uint4 *od = reinterpret_cast<uint4 *>(R.oDesc + 32 * o);
        od[0] = d[0]; od[1] = d[1];
    }
}

// ==== host side ==============================================================================================================================
bool frames_ok(const char *who, int n_frames) {
    if (n_frames < 1) { set_error("%s: n_frames %d below 1", who, n_frames); return false; }
    return true;
}
bool mcap_ok(const char *who, const char *name, int mcap) {
    if (mcap < 1 || mcap > MAX_MCAP) { set_error("%s: %s %d outside 1 .. %d", who, name, mcap, MAX_MCAP); return false; }
    return true;
}

const char *const WHO_KF = "msl_local_keyframes", *const WHO_PTS = "msl_local_points", *const WHO_LINES = "msl_local_lines";

int check_keyframes(int n_frames, int cap, int n_tab, int n_pts, int n_obs_total, int ccap, const int32_t *cur_held, const int32_t *n_cur,
                    const uint8_t *pt_flags, const int32_t *obs_off, const int32_t *obs_kf, const uint8_t *kf_flags, const int32_t *conn,
                    const int32_t *n_conn, const int32_t *parent, const int32_t *prev_kf, const int32_t *n_prev, msl_mem mem, int32_t *votes,
                    int32_t *local_kf, int32_t *n_local_kf, int32_t *ref_kf, uint8_t *cur_cleared, uint8_t *status, msl_mem) {
    const char *who = WHO_KF;
    if (!none_null(who, {MSL_NAMED(cur_held), MSL_NAMED(n_cur), MSL_NAMED(pt_flags), MSL_NAMED(obs_off), MSL_NAMED(obs_kf), MSL_NAMED(kf_flags),
                         MSL_NAMED(conn), MSL_NAMED(n_conn), MSL_NAMED(parent), MSL_NAMED(votes), MSL_NAMED(local_kf), MSL_NAMED(n_local_kf),
                         MSL_NAMED(ref_kf), MSL_NAMED(cur_cleared), MSL_NAMED(status)})) return MSL_ERR_INVALID;
    if (prev_kf && !n_prev) { set_error("%s: n_prev is NULL with prev_kf given", who); return MSL_ERR_INVALID; }
    if (!frames_ok(who, n_frames) || !table_limits(who, n_tab, cap, n_pts)) return MSL_ERR_INVALID;
    if (n_obs_total < 0) { set_error("%s: n_obs_total %d below 0", who, n_obs_total); return MSL_ERR_INVALID; }
    if (ccap < 1 || ccap > n_tab) { set_error("%s: ccap %d outside 1 .. n_tab = %d", who, ccap, n_tab); return MSL_ERR_INVALID; }
    char why[256];
    if (mem == MSL_MEM_HOST && (!check::csr_ok(n_tab, cap, n_pts, n_obs_total, obs_off, obs_kf, nullptr, nullptr, why, sizeof(why)) ||
                                !check::held_ok("cur_held", "n_cur", n_frames, cap, n_pts, cur_held, n_cur, why, sizeof(why)) ||
                                !check::graph_ok(n_tab, ccap, conn, n_conn, parent, why, sizeof(why)) ||
                                (prev_kf && !check::kf_rows_ok("prev_kf", "n_prev", "n_tab", n_frames, n_tab, n_tab, prev_kf, n_prev, why, sizeof(why)))))
        return refuse(who, why);
    return MSL_OK;
}

int launch_keyframes(msl_match *h, int n_frames, int cap, int n_tab, int n_pts, int n_obs_total, int ccap, const int32_t *cur_held,
                     const int32_t *n_cur, const uint8_t *pt_flags, const int32_t *obs_off, const int32_t *obs_kf, const uint8_t *kf_flags,
                     const int32_t *conn, const int32_t *n_conn, const int32_t *parent, const int32_t *prev_kf, const int32_t *n_prev, msl_mem mem,
                     int32_t *votes, int32_t *local_kf, int32_t *n_local_kf, int32_t *ref_kf, uint8_t *cur_cleared, uint8_t *status,
                     msl_mem out_mem) {
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    const size_t F = (size_t)n_frames, T = (size_t)n_tab, np = (size_t)n_pts, no = (size_t)n_obs_total;
    LocalKfDev D{};
    D.cap = cap; D.nTab = n_tab; D.nPts = n_pts; D.nObs = n_obs_total; D.ccap = ccap;
    Stage S(h, mem, out_mem);
    D.held = S.in(cur_held, F * cap); D.nCur = S.in(n_cur, F); D.flags = S.in(pt_flags, np);
    D.off = S.in(obs_off, np + 1); D.okf = S.in(no ? obs_kf : nullptr, no); D.kfFlags = S.in(kf_flags, T);
    D.conn = S.in(conn, T * ccap); D.nConn = S.in(n_conn, T); D.parent = S.in(parent, T);
    D.prev = S.in(prev_kf, F * T); D.nPrev = S.in(prev_kf ? n_prev : nullptr, F);
    D.votes = S.out(votes, F * T); D.list = S.out(local_kf, F * T); D.nList = S.out(n_local_kf, F); D.ref = S.out(ref_kf, F);
    D.cleared = S.out(cur_cleared, F * cap); D.status = S.out(status, F);
    MSL_HIP_TRY(S.error());
    hipLaunchKernelGGL(k_local_kf, dim3((unsigned)n_frames), dim3(LKF_NT), 0, h->stream, D);
    MSL_HIP_TRY(hipGetLastError());
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}

// What the point and the line entry share once their own limits are met: the NULLs, n_frames, the output capacity, the host-memory checks
struct RowNames { const char *who, *mcap, *held, *nKf, *cur, *nCur, *xyz, *normal, *dist, *desc, *flags, *nobs, *outId, *nOut, *oXyz, *oNormal, *oDist, *oDesc, *oFlags, *curFlags; };
const RowNames POINT_NAMES = {WHO_PTS, "mcap", "held_id", "n_kps", "cur_held", "n_cur", "pt_xyz", "pt_normal", "pt_dist", "pt_desc", "pt_flags", "pt_nobs",
                              "local_id", "n_local", "mp_xyz", "mp_normal", "mp_dist", "mp_desc", "mp_flags", "cur_flags"};
const RowNames LINE_NAMES = {WHO_LINES, "mlcap", "lheld_id", "n_kl", "cur_lheld", "n_cur_lines", "ln_xyz", "ln_normal", "ln_dist", "ln_desc", "ln_flags", "ln_nobs",
                             "local_line_id", "n_local_lines", "ml_xyz", "ml_normal", "ml_dist", "ml_desc", "ml_flags", "cur_line_flags"};

template <class T>
int check_rows(const RowNames &N, int n_frames, int n_tab, int fcap, int n_ids, int mcap, const int32_t *local_kf, const int32_t *n_local_kf,
               const int32_t *held, const int32_t *n_kf, const int32_t *cur, const int32_t *n_cur, const T *xyz, const T *normal, const float *dist,
               const uint8_t *desc, const uint8_t *flags, const int32_t *nobs, msl_mem mem, int32_t *out_id, int32_t *n_out, T *o_xyz, T *o_normal,
               float *o_dist, uint8_t *o_desc, uint8_t *o_flags, uint8_t *cur_flags) {
    if (!none_null(N.who, {{"local_kf", local_kf}, {"n_local_kf", n_local_kf}, {N.held, held}, {N.nKf, n_kf}, {N.cur, cur}, {N.nCur, n_cur},
                           {N.xyz, xyz}, {N.normal, normal}, {N.dist, dist}, {N.desc, desc}, {N.flags, flags}, {N.nobs, nobs}, {N.outId, out_id},
                           {N.nOut, n_out}, {N.oXyz, o_xyz}, {N.oNormal, o_normal}, {N.oDist, o_dist}, {N.oDesc, o_desc}, {N.oFlags, o_flags},
                           {N.curFlags, cur_flags}})) return MSL_ERR_INVALID;
    if (!frames_ok(N.who, n_frames) || !mcap_ok(N.who, N.mcap, mcap)) return MSL_ERR_INVALID;
    char why[256];
    if (mem == MSL_MEM_HOST && (!check::kf_rows_ok("local_kf", "n_local_kf", "n_tab", n_frames, n_tab, n_tab, local_kf, n_local_kf, why, sizeof(why)) ||
                                !check::held_ok(N.cur, N.nCur, n_frames, fcap, n_ids, cur, n_cur, why, sizeof(why)))) return refuse(N.who, why);
    return MSL_OK;
}

template <class T, int NX>
int launch_rows(msl_match *h, int n_frames, int n_tab, int kcap, int fcap, int n_ids, int mcap, const int32_t *local_kf, const int32_t *n_local_kf,
                const int32_t *held, const int32_t *n_kf, const int32_t *cur, const int32_t *n_cur, const T *xyz, const T *normal, const float *dist,
                const uint8_t *desc, const uint8_t *flags, const int32_t *nobs, msl_mem mem, int32_t *out_id, int32_t *n_out, T *o_xyz, T *o_normal,
                float *o_dist, uint8_t *o_desc, uint8_t *o_flags, uint8_t *cur_flags, msl_mem out_mem) {
    using W = typename std::conditional<sizeof(T) == 8, uint64_t, uint32_t>::type;   // rows are copied as words: bit for bit
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    const size_t F = (size_t)n_frames, Tn = (size_t)n_tab, ni = (size_t)n_ids, M = (size_t)mcap;
    size_t group = h->lmBudget / (4 * ni);                                     // frames whose stamps are in flight together
    group = group < 1 ? 1 : (group > F ? F : group);
    group = group > MAX_GROUP ? MAX_GROUP : group;
    LocalMapDev D{};
    LocalRows<W> R{};
    D.nTab = n_tab; D.kcap = kcap; D.fcap = fcap; D.nIds = n_ids; D.mcap = mcap;
    Stage S(h, mem, out_mem);
    D.list = S.in(local_kf, F * Tn); D.nList = S.in(n_local_kf, F); D.held = S.in(held, Tn * kcap); D.nKf = S.in(n_kf, Tn);
    D.cur = S.in(cur, F * fcap); D.nCur = S.in(n_cur, F);
    R.xyz = (const W *)S.in(xyz, NX * ni); R.normal = (const W *)S.in(normal, 3 * ni); R.dist = (const uint32_t *)S.in(dist, 2 * ni);
    R.desc = S.in(desc, 32 * ni); D.flags = S.in(flags, ni); D.nobs = S.in(nobs, ni);
    D.outId = S.out(out_id, F * M); D.nOut = S.out(n_out, F);
    // the rows beyond a frame's count keep their bytes, so a host-memory output is staged whole and copied back whole
    R.oXyz = (W *)S.inout(o_xyz, NX * F * M); R.oNormal = (W *)S.inout(o_normal, 3 * F * M); R.oDist = (uint32_t *)S.inout(o_dist, 2 * F * M);
    R.oDesc = S.inout(o_desc, 32 * F * M); D.outFlags = S.out(o_flags, F * M); D.curFlags = S.out(cur_flags, F * fcap);
    MSL_HIP_TRY(S.error());
    MSL_HIP_TRY(grow_all(h->stream, {{h->lmStamp, 4 * group * ni}, {h->lmCount, 4 * group * Tn}}));
    D.stamp = (unsigned *)h->lmStamp.p; D.count = (int32_t *)h->lmCount.p;
    for (size_t f0 = 0; f0 < F; f0 += group) {
        const unsigned G = (unsigned)(F - f0 < group ? F - f0 : group);
        D.f0 = (int)f0;
        MSL_HIP_TRY(hipMemsetAsync(D.stamp, 0xFF, 4 * (size_t)G * ni, h->stream));
        hipLaunchKernelGGL(k_lm_stamp, dim3((unsigned)n_tab, G), dim3(LM_NT), 0, h->stream, D);
        hipLaunchKernelGGL(k_lm_held, dim3((unsigned)((fcap + LM_NT - 1) / LM_NT), G), dim3(LM_NT), 0, h->stream, D);
        hipLaunchKernelGGL(k_lm_count, dim3((unsigned)n_tab, G), dim3(LM_NT), 0, h->stream, D);
        hipLaunchKernelGGL(k_lm_scan, dim3(G), dim3(LM_NT), 0, h->stream, D);
        hipLaunchKernelGGL((k_lm_write<W, NX>), dim3((unsigned)n_tab, G), dim3(LM_NT), 0, h->stream, D, R);
        MSL_HIP_TRY(hipGetLastError());
    }
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}

int check_points(int n_frames, int n_tab, int cap, int n_pts, int mcap, const int32_t *local_kf, const int32_t *n_local_kf, const int32_t *held_id,
                 const int32_t *n_kps, const int32_t *cur_held, const int32_t *n_cur, const float *pt_xyz, const float *pt_normal,
                 const float *pt_dist, const uint8_t *pt_desc, const uint8_t *pt_flags, const int32_t *pt_nobs, msl_mem mem, int32_t *local_id,
                 int32_t *n_local, float *mp_xyz, float *mp_normal, float *mp_dist, uint8_t *mp_desc, uint8_t *mp_flags, uint8_t *cur_flags, msl_mem) {
    if (!table_limits(WHO_PTS, n_tab, cap, n_pts)) return MSL_ERR_INVALID;
    return check_rows(POINT_NAMES, n_frames, n_tab, cap, n_pts, mcap, local_kf, n_local_kf, held_id, n_kps, cur_held, n_cur, pt_xyz, pt_normal,
                      pt_dist, pt_desc, pt_flags, pt_nobs, mem, local_id, n_local, mp_xyz, mp_normal, mp_dist, mp_desc, mp_flags, cur_flags);
}
int launch_points(msl_match *h, int n_frames, int n_tab, int cap, int n_pts, int mcap, const int32_t *local_kf, const int32_t *n_local_kf,
                  const int32_t *held_id, const int32_t *n_kps, const int32_t *cur_held, const int32_t *n_cur, const float *pt_xyz,
                  const float *pt_normal, const float *pt_dist, const uint8_t *pt_desc, const uint8_t *pt_flags, const int32_t *pt_nobs, msl_mem mem,
                  int32_t *local_id, int32_t *n_local, float *mp_xyz, float *mp_normal, float *mp_dist, uint8_t *mp_desc, uint8_t *mp_flags,
                  uint8_t *cur_flags, msl_mem out_mem) {
    return launch_rows<float, 3>(h, n_frames, n_tab, cap, cap, n_pts, mcap, local_kf, n_local_kf, held_id, n_kps, cur_held, n_cur, pt_xyz, pt_normal,
                                 pt_dist, pt_desc, pt_flags, pt_nobs, mem, local_id, n_local, mp_xyz, mp_normal, mp_dist, mp_desc, mp_flags,
                                 cur_flags, out_mem);
}

int check_lines(int n_frames, int n_tab, int klcap, int lcap, int n_lines, int mlcap, const int32_t *local_kf, const int32_t *n_local_kf,
                const int32_t *lheld_id, const int32_t *n_kl, const int32_t *cur_lheld, const int32_t *n_cur_lines, const double *ln_xyz,
                const double *ln_normal, const float *ln_dist, const uint8_t *ln_desc, const uint8_t *ln_flags, const int32_t *ln_nobs, msl_mem mem,
                int32_t *local_line_id, int32_t *n_local_lines, double *ml_xyz, double *ml_normal, float *ml_dist, uint8_t *ml_desc,
                uint8_t *ml_flags, uint8_t *cur_line_flags, msl_mem) {
    if (!line_table_limits(WHO_LINES, n_tab, klcap, n_lines)) return MSL_ERR_INVALID;
    if (lcap < 1 || lcap > MAX_KLCAP) { set_error("%s: lcap %d outside 1 .. %d", WHO_LINES, lcap, MAX_KLCAP); return MSL_ERR_INVALID; }
    return check_rows(LINE_NAMES, n_frames, n_tab, lcap, n_lines, mlcap, local_kf, n_local_kf, lheld_id, n_kl, cur_lheld, n_cur_lines, ln_xyz,
                      ln_normal, ln_dist, ln_desc, ln_flags, ln_nobs, mem, local_line_id, n_local_lines, ml_xyz, ml_normal, ml_dist, ml_desc,
                      ml_flags, cur_line_flags);
}
int launch_lines(msl_match *h, int n_frames, int n_tab, int klcap, int lcap, int n_lines, int mlcap, const int32_t *local_kf,
                 const int32_t *n_local_kf, const int32_t *lheld_id, const int32_t *n_kl, const int32_t *cur_lheld, const int32_t *n_cur_lines,
                 const double *ln_xyz, const double *ln_normal, const float *ln_dist, const uint8_t *ln_desc, const uint8_t *ln_flags,
                 const int32_t *ln_nobs, msl_mem mem, int32_t *local_line_id, int32_t *n_local_lines, double *ml_xyz, double *ml_normal,
                 float *ml_dist, uint8_t *ml_desc, uint8_t *ml_flags, uint8_t *cur_line_flags, msl_mem out_mem) {
    return launch_rows<double, 6>(h, n_frames, n_tab, klcap, lcap, n_lines, mlcap, local_kf, n_local_kf, lheld_id, n_kl, cur_lheld, n_cur_lines,
                                  ln_xyz, ln_normal, ln_dist, ln_desc, ln_flags, ln_nobs, mem, local_line_id, n_local_lines, ml_xyz, ml_normal,
                                  ml_dist, ml_desc, ml_flags, cur_line_flags, out_mem);
}

}  // namespace

extern "C" {

int msl_local_keyframes(msl_match *h, int n_frames, int cap, int n_tab, int n_pts, int n_obs_total, int ccap, const int32_t *cur_held,
                        const int32_t *n_cur, const uint8_t *pt_flags, const int32_t *obs_off, const int32_t *obs_kf, const uint8_t *kf_flags,
                        const int32_t *conn, const int32_t *n_conn, const int32_t *parent, const int32_t *prev_kf, const int32_t *n_prev,
                        msl_mem mem, int32_t *votes, int32_t *local_kf, int32_t *n_local_kf, int32_t *ref_kf, uint8_t *cur_cleared,
                        uint8_t *status, msl_mem out_mem) noexcept {
    try {
    return handle_form(WHO_KF, check_keyframes, launch_keyframes, h, n_frames, cap, n_tab, n_pts, n_obs_total, ccap, cur_held, n_cur, pt_flags,
                       obs_off, obs_kf, kf_flags, conn, n_conn, parent, prev_kf, n_prev, mem, votes, local_kf, n_local_kf, ref_kf, cur_cleared,
                       status, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_local_keyframes_batch(int device, int n_frames, int cap, int n_tab, int n_pts, int n_obs_total, int ccap, const int32_t *cur_held,
                              const int32_t *n_cur, const uint8_t *pt_flags, const int32_t *obs_off, const int32_t *obs_kf,
                              const uint8_t *kf_flags, const int32_t *conn, const int32_t *n_conn, const int32_t *parent, const int32_t *prev_kf,
                              const int32_t *n_prev, msl_mem mem, int32_t *votes, int32_t *local_kf, int32_t *n_local_kf, int32_t *ref_kf,
                              uint8_t *cur_cleared, uint8_t *status, msl_mem out_mem) noexcept {
    try {
    return batch_form(check_keyframes, launch_keyframes, device, mem == MSL_MEM_DEVICE, n_frames, cap, n_tab, n_pts, n_obs_total, ccap, cur_held,
                      n_cur, pt_flags, obs_off, obs_kf, kf_flags, conn, n_conn, parent, prev_kf, n_prev, mem, votes, local_kf, n_local_kf, ref_kf,
                      cur_cleared, status, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_local_points(msl_match *h, int n_frames, int n_tab, int cap, int n_pts, int mcap, const int32_t *local_kf, const int32_t *n_local_kf,
                     const int32_t *held_id, const int32_t *n_kps, const int32_t *cur_held, const int32_t *n_cur, const float *pt_xyz,
                     const float *pt_normal, const float *pt_dist, const uint8_t *pt_desc, const uint8_t *pt_flags, const int32_t *pt_nobs,
                     msl_mem mem, int32_t *local_id, int32_t *n_local, float *mp_xyz, float *mp_normal, float *mp_dist, uint8_t *mp_desc,
                     uint8_t *mp_flags, uint8_t *cur_flags, msl_mem out_mem) noexcept {
    try {
    return handle_form(WHO_PTS, check_points, launch_points, h, n_frames, n_tab, cap, n_pts, mcap, local_kf, n_local_kf, held_id, n_kps, cur_held,
                       n_cur, pt_xyz, pt_normal, pt_dist, pt_desc, pt_flags, pt_nobs, mem, local_id, n_local, mp_xyz, mp_normal, mp_dist, mp_desc,
                       mp_flags, cur_flags, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_local_points_batch(int device, int n_frames, int n_tab, int cap, int n_pts, int mcap, const int32_t *local_kf, const int32_t *n_local_kf,
                           const int32_t *held_id, const int32_t *n_kps, const int32_t *cur_held, const int32_t *n_cur, const float *pt_xyz,
                           const float *pt_normal, const float *pt_dist, const uint8_t *pt_desc, const uint8_t *pt_flags, const int32_t *pt_nobs,
                           msl_mem mem, int32_t *local_id, int32_t *n_local, float *mp_xyz, float *mp_normal, float *mp_dist, uint8_t *mp_desc,
                           uint8_t *mp_flags, uint8_t *cur_flags, msl_mem out_mem) noexcept {
    try {
    return batch_form(check_points, launch_points, device, mem == MSL_MEM_DEVICE, n_frames, n_tab, cap, n_pts, mcap, local_kf, n_local_kf, held_id,
                      n_kps, cur_held, n_cur, pt_xyz, pt_normal, pt_dist, pt_desc, pt_flags, pt_nobs, mem, local_id, n_local, mp_xyz, mp_normal,
                      mp_dist, mp_desc, mp_flags, cur_flags, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_local_lines(msl_match *h, int n_frames, int n_tab, int klcap, int lcap, int n_lines, int mlcap, const int32_t *local_kf,
                    const int32_t *n_local_kf, const int32_t *lheld_id, const int32_t *n_kl, const int32_t *cur_lheld, const int32_t *n_cur_lines,
                    const double *ln_xyz, const double *ln_normal, const float *ln_dist, const uint8_t *ln_desc, const uint8_t *ln_flags,
                    const int32_t *ln_nobs, msl_mem mem, int32_t *local_line_id, int32_t *n_local_lines, double *ml_xyz, double *ml_normal,
                    float *ml_dist, uint8_t *ml_desc, uint8_t *ml_flags, uint8_t *cur_line_flags, msl_mem out_mem) noexcept {
    try {
    return handle_form(WHO_LINES, check_lines, launch_lines, h, n_frames, n_tab, klcap, lcap, n_lines, mlcap, local_kf, n_local_kf, lheld_id, n_kl,
                       cur_lheld, n_cur_lines, ln_xyz, ln_normal, ln_dist, ln_desc, ln_flags, ln_nobs, mem, local_line_id, n_local_lines, ml_xyz,
                       ml_normal, ml_dist, ml_desc, ml_flags, cur_line_flags, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_local_lines_batch(int device, int n_frames, int n_tab, int klcap, int lcap, int n_lines, int mlcap, const int32_t *local_kf,
                          const int32_t *n_local_kf, const int32_t *lheld_id, const int32_t *n_kl, const int32_t *cur_lheld,
                          const int32_t *n_cur_lines, const double *ln_xyz, const double *ln_normal, const float *ln_dist, const uint8_t *ln_desc,
                          const uint8_t *ln_flags, const int32_t *ln_nobs, msl_mem mem, int32_t *local_line_id, int32_t *n_local_lines,
                          double *ml_xyz, double *ml_normal, float *ml_dist, uint8_t *ml_desc, uint8_t *ml_flags, uint8_t *cur_line_flags,
                          msl_mem out_mem) noexcept {
    try {
    return batch_form(check_lines, launch_lines, device, mem == MSL_MEM_DEVICE, n_frames, n_tab, klcap, lcap, n_lines, mlcap, local_kf, n_local_kf,
                      lheld_id, n_kl, cur_lheld, n_cur_lines, ln_xyz, ln_normal, ln_dist, ln_desc, ln_flags, ln_nobs, mem, local_line_id,
                      n_local_lines, ml_xyz, ml_normal, ml_dist, ml_desc, ml_flags, cur_line_flags, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_debug_local_map_budget(msl_match *h, size_t bytes) noexcept {
    try {
    if (!h || bytes < 4) { set_error("msl_debug_local_map_budget: invalid argument (null handle, or fewer than 4 bytes)"); return MSL_ERR_INVALID; }
    h->lmBudget = bytes;
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}

}  // extern "C"

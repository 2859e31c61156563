// msl_cull.hip -- the four cullings of LocalMapping::Run for gfx950: LocalMapping::KeyFrameCulling (reference src/LocalMapping.cc:704-759) as
// msl_cull_keyframes[_batch], and the elementwise verdict of MapPointCulling / MapLineCulling / MapPlaneCulling (:227-301) as
// msl_cull_recent[_batch].
//   k_cull_kf      one workgroup of 1024 per item walks the item's candidates in order.  Threads stride over the candidate's slots and each
//                  walks its point's observation range once: that pass gives the point's current nObs, whether it has turned bad, and the
//                  count of qualifying observations together.  The only state an item carries from one candidate to the next is an LDS
//                  bitmap of the keyframes culled so far: an observation (k, idx) of p is gone iff k is in the bitmap and k holds p.  No
//                  atomics, no table-sized scratch; two barriers per candidate
//   k_cull_recent  one thread per recent element
// "k holds p" is held_id[k][idx] == p at the observation's own index; only on a mismatch are k's slots scanned (inconsistent tables).
// Pins (tests/cull_model.py is the sequential model): msl.h's list; device-only: an index outside its table is absent.
#include "msl_match_handle.h"
#include "msl_index_check.h"
#include "msl_obs_walk.h"

namespace {

using namespace msl;

constexpr int CULL_NT = 1024, RECENT_NT = 256, MAX_ITEMS = 4096, MAX_RECENT = 1 << 20;
constexpr int TH_OBS = 3;                                                      // thObs of :719
static_assert(MAX_CAP * 10 < (1 << 30), "10 * n_redundant > 9 * n_mps is taken in int");

// ==== KeyFrameCulling of one item ============================================================================================================
struct CullDev {
    int nTab, cap, nPts, nObs, ccap, origin;
    float thDepth;
    const msl_keypoint *kps; const float *uright, *depth; const int32_t *held, *nKps; const uint8_t *kfFlags, *flags; const int32_t *ptNobs;
    const int32_t *off, *okf, *oidx, *cand, *nCand;
    int32_t *nMps, *nRed, *nGone; uint8_t *status;
};

// Whether keyframe k holds point p in some slot below its count; idx: the index of p's observation by k, where a consistent table has it
__device__ __forceinline__ bool kf_holds(const CullDev &D, int k, int idx, int p) {
    const int n = clampi(D.nKps[k], 0, D.cap);
    const int32_t *row = D.held + (size_t)k * D.cap;
    if (idx < n && row[idx] == p) return true;
    for (int i = 0; i < n; i++)
        if (row[i] == p) return true;
    return false;
}

__global__ __launch_bounds__(CULL_NT) void k_cull_kf(CullDev D) {
    __shared__ unsigned s_culled[MAX_TAB / 32];                                // the keyframes whose SetBadFlag took effect so far
    __shared__ int s_part[CULL_NT / WAVE][3];
    const int f = blockIdx.x, lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    for (int j = threadIdx.x; j < MAX_TAB / 32; j += CULL_NT) s_culled[j] = 0u;
    const int nc = clampi(D.nCand[f], 0, D.ccap);
    for (int r = nc + threadIdx.x; r < D.ccap; r += CULL_NT) {
        const size_t o = (size_t)f * D.ccap + r;
        D.nMps[o] = -1; D.nRed[o] = -1; D.nGone[o] = -1; D.status[o] = 0;
    }
    __syncthreads();
    for (int r = 0; r < nc; r++) {
        const size_t out = (size_t)f * D.ccap + r;
        const int c = D.cand[out];
        if (c < 0 || c >= D.nTab || c == D.origin) {                           // uniform: the whole workgroup skips (:715)
            if (threadIdx.x == 0) {
                D.nMps[out] = 0; D.nRed[out] = 0; D.nGone[out] = 0;
                D.status[out] = c < 0 || c >= D.nTab ? MSL_CULL_ABSENT : MSL_CULL_ORIGIN;
            }
            continue;
        }
        const int n = clampi(D.nKps[c], 0, D.cap);
        int mps = 0, red = 0, gone = 0;
        for (int i = threadIdx.x; i < n; i += CULL_NT) {
            const size_t slot = (size_t)c * D.cap + i;
            const int p = D.held[slot];
            if (p < 0 || p >= D.nPts || !(D.flags[p] & 1)) continue;           // NULL, or bad on entry
            const int level = D.kps[slot].octave;
            int nobs = D.ptNobs[p], cnt = 0, b, e;
            bool erased = false;
            obs_range(D, p, b, e);
            for (int o = b; o < e; o++) {
                const int k = D.okf[o], idx = D.oidx[o];
                if (k < 0 || k >= D.nTab || idx < 0 || idx >= D.cap) continue; // absent
                const size_t kp = (size_t)k * D.cap + idx;
                if ((s_culled[k >> 5] >> (k & 31) & 1u) && kf_holds(D, k, idx, p)) {
                    nobs -= D.uright[kp] >= 0 ? 2 : 1;                         // EraseObservation: the observation's own keypoint
                    erased = true;
                } else if (k != c && D.kps[kp].octave <= level + 1) {
                    cnt++;
                }
            }
            if (erased && nobs <= 2) { gone++; continue; }                     // turned bad at one of the erasures: nObs only falls
            const float d = D.depth[slot];
            if (d > D.thDepth || d < 0) continue;                              // the literal tests: a NaN depth counts
            mps++;
            red += nobs > TH_OBS && cnt >= TH_OBS;
        }
        mps = wave_sum(mps); red = wave_sum(red); gone = wave_sum(gone);
        if (lane == 0) { s_part[wave][0] = mps; s_part[wave][1] = red; s_part[wave][2] = gone; }
        __syncthreads();
        if (threadIdx.x == 0) {
            mps = red = gone = 0;
            for (int w = 0; w < CULL_NT / WAVE; w++) { mps += s_part[w][0]; red += s_part[w][1]; gone += s_part[w][2]; }
            // (double)red > 0.9 * (double)mps for every mps <= 8192; mps == 0 keeps the keyframe
            const bool redundant = 10 * red > 9 * mps;
            const bool held_back = D.kfFlags[c] & 2;                           // mbNotErase: SetBadFlag returns at src/KeyFrame.cc:354
            if (redundant && !held_back) s_culled[c >> 5] |= 1u << (c & 31);
            D.nMps[out] = mps; D.nRed[out] = red; D.nGone[out] = gone;
            D.status[out] = !redundant ? MSL_CULL_KEPT : held_back ? MSL_CULL_NOT_ERASE : MSL_CULL_CULLED;
        }
        __syncthreads();
    }
}

// ==== MapPointCulling / MapLineCulling / MapPlaneCulling: the verdict of one recent element ===================================================
struct RecentDev {
    int n, curKfId, thObs, intForm;
    const int32_t *found, *visible, *firstKfId, *nobs; const uint8_t *flags;
    uint8_t *verdict;
};

__global__ __launch_bounds__(RECENT_NT) void k_cull_recent(RecentDev D) {
    const int i = blockIdx.x * RECENT_NT + threadIdx.x;
    if (i >= D.n) return;
    int v = MSL_RECENT_KEEP;
    const int found = D.found[i], visible = D.visible[i], age = D.curKfId - D.firstKfId[i];
    if (!(D.flags[i] & 1)) {
        v = MSL_RECENT_ERASE_BAD;
    } else if (D.intForm && visible == 0) {
        v = MSL_RECENT_INVALID;
    } else {
        // src/MapPoint.cc:205 and src/MapPlane.cc:173 divide floats; src/MapLine.cpp:190-193 casts the integer quotient
        const float ratio = D.intForm ? (float)((long long)found / (long long)visible) : (float)found / (float)visible;
        if (ratio < 0.25f) v = MSL_RECENT_CULL_RATIO;
        else if (age >= 2 && D.nobs[i] <= D.thObs) v = MSL_RECENT_CULL_OBS;
        else if (age >= 3) v = MSL_RECENT_RETIRE;
    }
    D.verdict[i] = (uint8_t)v;
}

// ==== host side ==============================================================================================================================
const char *const WHO_KF = "msl_cull_keyframes", *const WHO_RECENT = "msl_cull_recent";

int check_keyframes(int n_tab, int cap, int n_pts, int n_items, int n_obs_total, int ccap, int origin, const msl_cull_params *params,
                    const msl_keypoint *kps_un, const float *uright, const float *depth, const int32_t *held_id, const int32_t *n_kps,
                    const uint8_t *kf_flags, const uint8_t *pt_flags, const int32_t *pt_nobs, const int32_t *obs_off, const int32_t *obs_kf,
                    const int32_t *obs_idx, const int32_t *cand, const int32_t *n_cand, msl_mem mem, int32_t *n_mps, int32_t *n_redundant,
                    int32_t *n_gone, uint8_t *status, msl_mem) {
    const char *who = WHO_KF;
    if (!none_null(who, {MSL_NAMED(params), MSL_NAMED(kps_un), MSL_NAMED(uright), MSL_NAMED(depth), MSL_NAMED(held_id), MSL_NAMED(n_kps),
                         MSL_NAMED(kf_flags), MSL_NAMED(pt_flags), MSL_NAMED(pt_nobs), MSL_NAMED(obs_off), MSL_NAMED(obs_kf), MSL_NAMED(obs_idx),
                         MSL_NAMED(cand), MSL_NAMED(n_cand), MSL_NAMED(n_mps), MSL_NAMED(n_redundant), MSL_NAMED(n_gone), MSL_NAMED(status)}))
        return MSL_ERR_INVALID;
    if (!table_limits(who, n_tab, cap, n_pts)) return MSL_ERR_INVALID;
    if (n_items < 1 || n_items > MAX_ITEMS) { set_error("%s: n_items %d outside 1 .. %d", who, n_items, MAX_ITEMS); return MSL_ERR_INVALID; }
    if (n_obs_total < 0) { set_error("%s: n_obs_total %d below 0", who, n_obs_total); return MSL_ERR_INVALID; }
    if (ccap < 1 || ccap > n_tab) { set_error("%s: ccap %d outside 1 .. n_tab = %d", who, ccap, n_tab); return MSL_ERR_INVALID; }
    char why[256];
    if (mem == MSL_MEM_HOST && (!check::origin_ok(n_tab, origin, why, sizeof(why)) ||
                                !check::csr_ok(n_tab, cap, n_pts, n_obs_total, obs_off, obs_kf, obs_idx, n_kps, why, sizeof(why)) ||
                                !check::kf_rows_ok("cand", "n_cand", "ccap", n_items, n_tab, ccap, cand, n_cand, why, sizeof(why))))
        return refuse(who, why);
    return MSL_OK;
}

int launch_keyframes(msl_match *h, int n_tab, int cap, int n_pts, int n_items, int n_obs_total, int ccap, int origin,
                     const msl_cull_params *params, const msl_keypoint *kps_un, const float *uright, const float *depth, const int32_t *held_id,
                     const int32_t *n_kps, const uint8_t *kf_flags, const uint8_t *pt_flags, const int32_t *pt_nobs, const int32_t *obs_off,
                     const int32_t *obs_kf, const int32_t *obs_idx, const int32_t *cand, const int32_t *n_cand, msl_mem mem, int32_t *n_mps,
                     int32_t *n_redundant, int32_t *n_gone, uint8_t *status, msl_mem out_mem) {
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    const size_t T = (size_t)n_tab, np = (size_t)n_pts, no = (size_t)n_obs_total, FC = (size_t)n_items * ccap;
    CullDev D{};
    D.nTab = n_tab; D.cap = cap; D.nPts = n_pts; D.nObs = n_obs_total; D.ccap = ccap; D.thDepth = params->th_depth;
    D.origin = origin >= 0 && origin < n_tab ? origin : -1;
    Stage S(h, mem, out_mem);
    D.kps = S.in(kps_un, T * cap); D.uright = S.in(uright, T * cap); D.depth = S.in(depth, T * cap); D.held = S.in(held_id, T * cap);
    D.nKps = S.in(n_kps, T); D.kfFlags = S.in(kf_flags, T); D.flags = S.in(pt_flags, np); D.ptNobs = S.in(pt_nobs, np);
    D.off = S.in(obs_off, np + 1); D.okf = S.in(no ? obs_kf : nullptr, no); D.oidx = S.in(no ? obs_idx : nullptr, no);
    D.cand = S.in(cand, FC); D.nCand = S.in(n_cand, (size_t)n_items);
    D.nMps = S.out(n_mps, FC); D.nRed = S.out(n_redundant, FC); D.nGone = S.out(n_gone, FC); D.status = S.out(status, FC);
    MSL_HIP_TRY(S.error());
    hipLaunchKernelGGL(k_cull_kf, dim3((unsigned)n_items), dim3(CULL_NT), 0, h->stream, D);
    MSL_HIP_TRY(hipGetLastError());
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}

int check_recent(int n, int cur_kf_id, int th_obs, int ratio_form, const int32_t *found, const int32_t *visible, const int32_t *first_kf_id,
                 const int32_t *nobs, const uint8_t *flags, msl_mem mem, uint8_t *verdict, msl_mem) {
    const char *who = WHO_RECENT;
    if (!none_null(who, {MSL_NAMED(found), MSL_NAMED(visible), MSL_NAMED(first_kf_id), MSL_NAMED(nobs), MSL_NAMED(flags), MSL_NAMED(verdict)}))
        return MSL_ERR_INVALID;
    if (n < 1 || n > MAX_RECENT) { set_error("%s: n %d outside 1 .. %d", who, n, MAX_RECENT); return MSL_ERR_INVALID; }
    if (cur_kf_id < 0) { set_error("%s: cur_kf_id %d below 0", who, cur_kf_id); return MSL_ERR_INVALID; }
    if (th_obs < 0) { set_error("%s: th_obs %d below 0", who, th_obs); return MSL_ERR_INVALID; }
    if (ratio_form != MSL_RATIO_FLOAT && ratio_form != MSL_RATIO_INT) {
        set_error("%s: ratio_form %d is neither MSL_RATIO_FLOAT nor MSL_RATIO_INT", who, ratio_form);
        return MSL_ERR_INVALID;
    }
    char why[256];
    if (mem == MSL_MEM_HOST && !check::recent_ok(n, ratio_form == MSL_RATIO_INT, found, visible, first_kf_id, flags, why, sizeof(why)))
        return refuse(who, why);
    return MSL_OK;
}

int launch_recent(msl_match *h, int n, int cur_kf_id, int th_obs, int ratio_form, const int32_t *found, const int32_t *visible,
                  const int32_t *first_kf_id, const int32_t *nobs, const uint8_t *flags, msl_mem mem, uint8_t *verdict, msl_mem out_mem) {
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    const size_t N = (size_t)n;
    RecentDev D{};
    D.n = n; D.curKfId = cur_kf_id; D.thObs = th_obs; D.intForm = ratio_form == MSL_RATIO_INT;
    Stage S(h, mem, out_mem);
    D.found = S.in(found, N); D.visible = S.in(visible, N); D.firstKfId = S.in(first_kf_id, N); D.nobs = S.in(nobs, N); D.flags = S.in(flags, N);
    D.verdict = S.out(verdict, N);
    MSL_HIP_TRY(S.error());
    hipLaunchKernelGGL(k_cull_recent, dim3((unsigned)((n + RECENT_NT - 1) / RECENT_NT)), dim3(RECENT_NT), 0, h->stream, D);
    MSL_HIP_TRY(hipGetLastError());
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}

}  // namespace

extern "C" {

int msl_cull_keyframes(msl_match *h, int n_tab, int cap, int n_pts, int n_items, int n_obs_total, int ccap, int origin,
                       const msl_cull_params *params, const msl_keypoint *kps_un, const float *uright, const float *depth,
                       const int32_t *held_id, const int32_t *n_kps, const uint8_t *kf_flags, const uint8_t *pt_flags, const int32_t *pt_nobs,
                       const int32_t *obs_off, const int32_t *obs_kf, const int32_t *obs_idx, const int32_t *cand, const int32_t *n_cand,
                       msl_mem mem, int32_t *n_mps, int32_t *n_redundant, int32_t *n_gone, uint8_t *status, msl_mem out_mem) noexcept {
    try {
    return handle_form(WHO_KF, check_keyframes, launch_keyframes, h, n_tab, cap, n_pts, n_items, n_obs_total, ccap, origin, params, kps_un, uright,
                       depth, held_id, n_kps, kf_flags, pt_flags, pt_nobs, obs_off, obs_kf, obs_idx, cand, n_cand, mem, n_mps, n_redundant, n_gone,
                       status, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_cull_keyframes_batch(int device, int n_tab, int cap, int n_pts, int n_items, int n_obs_total, int ccap, int origin,
                             const msl_cull_params *params, const msl_keypoint *kps_un, const float *uright, const float *depth,
                             const int32_t *held_id, const int32_t *n_kps, const uint8_t *kf_flags, const uint8_t *pt_flags,
                             const int32_t *pt_nobs, const int32_t *obs_off, const int32_t *obs_kf, const int32_t *obs_idx, const int32_t *cand,
                             const int32_t *n_cand, msl_mem mem, int32_t *n_mps, int32_t *n_redundant, int32_t *n_gone, uint8_t *status,
                             msl_mem out_mem) noexcept {
    try {
    return batch_form(check_keyframes, launch_keyframes, device, mem == MSL_MEM_DEVICE, n_tab, cap, n_pts, n_items, n_obs_total, ccap, origin,
                      params, kps_un, uright, depth, held_id, n_kps, kf_flags, pt_flags, pt_nobs, obs_off, obs_kf, obs_idx, cand, n_cand, mem, n_mps,
                      n_redundant, n_gone, status, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_cull_recent(msl_match *h, int n, int cur_kf_id, int th_obs, int ratio_form, const int32_t *found, const int32_t *visible,
                    const int32_t *first_kf_id, const int32_t *nobs, const uint8_t *flags, msl_mem mem, uint8_t *verdict,
                    msl_mem out_mem) noexcept {
    try {
    return handle_form(WHO_RECENT, check_recent, launch_recent, h, n, cur_kf_id, th_obs, ratio_form, found, visible, first_kf_id, nobs, flags, mem,
                       verdict, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_cull_recent_batch(int device, int n, int cur_kf_id, int th_obs, int ratio_form, const int32_t *found, const int32_t *visible,
                          const int32_t *first_kf_id, const int32_t *nobs, const uint8_t *flags, msl_mem mem, uint8_t *verdict,
                          msl_mem out_mem) noexcept {
    try {
    return batch_form(check_recent, launch_recent, device, mem == MSL_MEM_DEVICE, n, cur_kf_id, th_obs, ratio_form, found, visible, first_kf_id,
                      nobs, flags, mem, verdict, out_mem);
    } MSL_ABI_CATCH_INT
}

}  // extern "C"

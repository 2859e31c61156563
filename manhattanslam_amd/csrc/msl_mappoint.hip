// msl_mappoint.hip -- what LocalMapping does with its map points and keyframe right after the fusion, for gfx950: MapPoint::
// ComputeDistinctiveDescriptors (reference src/MapPoint.cc:210-270) and MapPoint::UpdateNormalAndDepth (:282-322) as
// msl_refresh_map_points[_batch], the counting and ordering of KeyFrame::UpdateConnections (src/KeyFrame.cc:230-299) as msl_covisibility[_batch].
// Both read the observations as CSR over the point table (msl.h); the caller's order inside a point's range is the map's iteration order.
//   k_refresh  one wave per point.  Its observations are walked 64 at a time: the descriptors of the live keyframes are compacted into
//              LDS in list order (8 KB for MSL_OBS_MAX = 256), the normal's terms are formed by the lanes and added in list order, the same
//              sum in every lane.  Then lane i owns the rows i, i + 64, ... of the distance matrix: the median of a row is its k-th
//              smallest value, found by bisecting the value range 0 .. 256 in nine counting passes over the LDS descriptors (every lane
//              reads the same descriptor at the same time, a broadcast) -- no per-lane sort, no distance matrix.  The winner is the wave
//              minimum of (median << 8 | row): the first row with a strictly smaller median
//   k_covis    one workgroup per keyframe: a counter per table keyframe in LDS (16 KB at 4096), one LDS atomicAdd per observation of a held
//              point; the counters >= th compacted into (weight << 12 | index) keys, sorted ascending and written back to front (descending
//              weight, then descending index, as sort + push_front leaves them); the fallback is the maximum of (weight << 12 | 4095 - index)
// Pins (tests/mappoint_model.py is the sequential model; contraction off): the arithmetic of msl.h's list; device-only: an observation whose
// keyframe is outside the table is skipped as if absent, one whose keypoint index is outside [0, cap) has no descriptor; an id outside the
// point table is a bad point; a pt_ref outside the table, or a reference keypoint outside [0, cap), leaves as MSL_REFRESH_BAD_OCTAVE.
#include "msl_match_handle.h"
#include "msl_index_check.h"
#include "msl_obs_walk.h"

namespace {

using namespace msl;

constexpr int COVIS_NT = 1024, IDX_BITS = 12;
static_assert(MAX_TAB == 1 << IDX_BITS && (MSL_OBS_MAX & (MSL_OBS_MAX - 1)) == 0 && MSL_OBS_MAX <= 256, "key layouts");

struct RefreshDev {
    int nTab, cap, nPts, nObs, what;
    msl_refresh_params prm;
    const msl_keypoint *kps; const uint8_t *desc; const float *Tcw; const uint8_t *kfFlags;
    const int32_t *off, *okf, *oidx;
    const float *xyz; const uint8_t *flags; const int32_t *ref, *ids;
    uint8_t *outDesc; float *outNormal, *outDist; int32_t *bestObs, *bestMedian; uint8_t *status;
    uint8_t *ptDesc; float *ptNormal, *ptDist;
};

// v = X - Ow of keyframe pose T, in float; returns cv::norm(v), the square root of a double sum
__device__ __forceinline__ double view_vector(const float *T, const float X[3], float v[3]) {
    float Ow[3];
    camera_centre(T, Ow);
#pragma unroll
    for (int a = 0; a < 3; a++) v[a] = X[a] - Ow[a];
    return norm3_dacc(v);
}

// ==== ComputeDistinctiveDescriptors and UpdateNormalAndDepth of one point ====================================================================
__global__ __launch_bounds__(WAVE) void k_refresh(RefreshDev D) {
    __shared__ uint4 s_desc[2 * MSL_OBS_MAX];                                  // the live descriptors in list order
    __shared__ int s_pos[MSL_OBS_MAX];                                         // their positions in the point's own observation range
    const int f = blockIdx.x, lane = threadIdx.x;
    const int id = D.ids[f];
    const bool wantD = D.what & MSL_REFRESH_DESC, wantN = D.what & MSL_REFRESH_NORMAL;
    int status = MSL_REFRESH_BAD, bestObs = -1, bestMedian = 0;
    uint4 d0 = make_uint4(0, 0, 0, 0), d1 = d0;
    float normal[3] = {0.0f, 0.0f, 0.0f}, dist[2] = {0.0f, 0.0f};
    if (id >= 0 && id < D.nPts && (D.flags[id] & 1)) {                         // uniform, as every branch outside the lane loops
        int b, e;
        obs_range(D, id, b, e);
        const int ref = wantN ? D.ref[id] : -1;
        float X[3] = {0.0f, 0.0f, 0.0f};
        if (wantN) { X[0] = D.xyz[3 * (size_t)id]; X[1] = D.xyz[3 * (size_t)id + 1]; X[2] = D.xyz[3 * (size_t)id + 2]; }
        int n = 0, nLive = 0, refIdx = 0;                                      // refIdx 0: map::operator[] of an absent key
        bool refSeen = false;
        float acc[3] = {0.0f, 0.0f, 0.0f};
        for (int c = b; c < e; c += WAVE) {
            const int o = c + lane;
            // obs_chunk of msl_obs_walk.h, written out: around the shared form the compiler swaps operands in this kernel's pinned text
            int k = -1, idx = -1;
            if (o < e) { k = D.okf[o]; idx = D.oidx[o]; }
            const bool valid = k >= 0 && k < D.nTab;
            const unsigned long long m = __ballot(valid);
            n += __popcll(m);
            if (wantD) {
                const bool live = valid && (D.kfFlags[k] & 1) && idx >= 0 && idx < D.cap;
                const unsigned long long ml = __ballot(live);
                const int r = nLive + __popcll(ml & ((1ull << lane) - 1ull));
                if (live && r < MSL_OBS_MAX) {
                    load_desc(D.desc + ((size_t)k * D.cap + idx) * 32, s_desc[2 * r], s_desc[2 * r + 1]);
                    s_pos[r] = o - b;
                }
                nLive += __popcll(ml);
            }
            if (wantN) {
                float t[3] = {0.0f, 0.0f, 0.0f};
                if (valid) {
                    float v[3];
                    const double inv = 1.0 / view_vector(D.Tcw + (size_t)k * 12, X, v);
#pragma unroll
                    for (int a = 0; a < 3; a++) t[a] = (float)((double)v[a] * inv);
                }
                const unsigned long long mr = __ballot(valid && k == ref);     // obs_ref_index, written out as obs_chunk above
                if (!refSeen && mr) { refIdx = __shfl(idx, __ffsll(mr) - 1); refSeen = true; }
                obs_add_in_order(m, t, acc);                                   // normal = normal + normali / norm, in list order
            }
        }
        status = MSL_REFRESH_NO_OBS;
        if (n > 0) {
            status = 0;
            if (wantD && nLive == 0) status |= MSL_REFRESH_NO_LIVE_KF;
            else if (wantD && nLive > MSL_OBS_MAX) status |= MSL_REFRESH_TOO_MANY;
            else if (wantD) {
                __syncthreads();
                const int N = nLive, kth = (int)(0.5 * (N - 1));
                unsigned key = ~0u;
                for (int r = lane; r < N; r += WAVE) {
                    const uint4 a0 = s_desc[2 * r], a1 = s_desc[2 * r + 1];
                    int lo = 0, hi = 256;                                      // the smallest v with more than kth distances <= v
                    for (int it = 0; it < 9; it++) {
                        const int mid = (lo + hi) >> 1;
                        int cnt = 0;
                        for (int j = 0; j < N; j++) cnt += hamming256(a0, a1, s_desc[2 * j], s_desc[2 * j + 1]) <= mid ? 1 : 0;
                        if (cnt > kth) hi = mid; else lo = mid + 1;
                    }
                    const unsigned kk = ((unsigned)lo << 8) | (unsigned)r;
                    key = kk < key ? kk : key;
                }
                key = wave_min(key);
                const int best = (int)(key & 255u);
                bestMedian = (int)(key >> 8); bestObs = s_pos[best];
                d0 = s_desc[2 * best]; d1 = s_desc[2 * best + 1];
                status |= MSL_REFRESH_DESC_WRITTEN;
            }
            if (wantN) {
                int level = -1;
                if (ref >= 0 && ref < D.nTab && refIdx >= 0 && refIdx < D.cap) level = D.kps[(size_t)ref * D.cap + refIdx].octave;
                if (level < 0 || level >= D.prm.nlevels) status |= MSL_REFRESH_BAD_OCTAVE;
                else {
                    float PC[3];
                    const float d = (float)view_vector(D.Tcw + (size_t)ref * 12, X, PC);
                    dist[1] = d * D.prm.scale_factors[level];
                    dist[0] = dist[1] / D.prm.scale_factors[D.prm.nlevels - 1];
                    const double invn = 1.0 / (double)n;
#pragma unroll
                    for (int a = 0; a < 3; a++) normal[a] = (float)((double)acc[a] * invn);
                    status |= MSL_REFRESH_NORMAL_WRITTEN;
                }
            }
        }
    }
    if (lane < 2) {
        const uint4 d = lane ? d1 : d0;
        reinterpret_cast<uint4 *>(D.outDesc + (size_t)f * 32)[lane] = d;
        if (D.ptDesc && (status & MSL_REFRESH_DESC_WRITTEN)) reinterpret_cast<uint4 *>(D.ptDesc + (size_t)id * 32)[lane] = d;
    }
    if (lane == 0) {
        D.bestObs[f] = bestObs; D.bestMedian[f] = bestMedian; D.status[f] = (uint8_t)status;
        const bool wrote = status & MSL_REFRESH_NORMAL_WRITTEN;
#pragma unroll
        for (int a = 0; a < 3; a++) {                                          // write_item_and_row, written out as the other two
            D.outNormal[3 * (size_t)f + a] = normal[a];
            if (D.ptNormal && wrote) D.ptNormal[3 * (size_t)id + a] = normal[a];
        }
#pragma unroll
        for (int a = 0; a < 2; a++) {
            D.outDist[2 * (size_t)f + a] = dist[a];
            if (D.ptDist && wrote) D.ptDist[2 * (size_t)id + a] = dist[a];
        }
    }
}

// ==== KFcounter and the ordered connections of one keyframe ==================================================================================
struct CovisDev {
    int nTab, cap, nPts, nObs, ccap, th, P;
    const int32_t *held, *n; const uint8_t *flags; const int32_t *off, *okf, *kf;
    int32_t *weight, *conn, *connW, *nConn;
};

__global__ __launch_bounds__(COVIS_NT) void k_covis(CovisDev D) {
    extern __shared__ unsigned long long s_key[];                              // [P] keys, then [nTab] counters
    __shared__ unsigned s_n;
    __shared__ unsigned long long s_max;
    unsigned *s_cnt = reinterpret_cast<unsigned *>(s_key + D.P);
    const int f = blockIdx.x, k = D.kf[f];
    for (int j = threadIdx.x; j < D.P; j += COVIS_NT) s_key[j] = ~0ull;
    for (int j = threadIdx.x; j < D.nTab; j += COVIS_NT) s_cnt[j] = 0;
    if (threadIdx.x == 0) { s_n = 0; s_max = 0; }
    __syncthreads();
    if (k >= 0 && k < D.nTab) {
        const int n = clampi(D.n[k], 0, D.cap);
        for (int i = threadIdx.x; i < n; i += COVIS_NT) {
            const int id = D.held[(size_t)k * D.cap + i];
            if (id < 0 || id >= D.nPts || !(D.flags[id] & 1)) continue;
            const int b = clampi(D.off[id], 0, D.nObs), e = clampi(D.off[id + 1], b, D.nObs);   // obs_range, written out (msl_obs_walk.h)
            for (int o = b; o < e; o++) {
                const int kk = D.okf[o];
                if (kk >= 0 && kk < D.nTab && kk != k) atomicAdd(&s_cnt[kk], 1u);      // a bad observer counts: the reference has no test
            }
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < D.nTab; j += COVIS_NT) {
        const unsigned w = s_cnt[j];
        D.weight[(size_t)f * D.nTab + j] = (int)w;
        if (w == 0) continue;
        atomicMax(&s_max, ((unsigned long long)w << IDX_BITS) | (unsigned)(MAX_TAB - 1 - j));   // strict > in ascending order: the lowest index
        if ((long long)w >= (long long)D.th) s_key[atomicAdd(&s_n, 1u)] = ((unsigned long long)w << IDX_BITS) | (unsigned)j;
    }
    __syncthreads();
    int cnt = (int)s_n;
    const unsigned long long mx = s_max;
    if (cnt == 0 && mx != 0) {                                                 // vPairs.empty(): the keyframe of maximum weight alone
        if (threadIdx.x == 0) s_key[0] = (mx & ~(unsigned long long)(MAX_TAB - 1)) | (unsigned)(MAX_TAB - 1 - (int)(mx & (MAX_TAB - 1)));
        cnt = 1;
    }
    bitonic_sort(s_key, pow2_at_least(cnt > 2 ? cnt : 2));                     // ascending (weight, index); the rest of s_key is ~0
    for (int r = threadIdx.x; r < D.ccap; r += COVIS_NT) {
        const bool has = r < cnt;
        const unsigned long long key = has ? s_key[cnt - 1 - r] : 0ull;        // push_front
        D.conn[(size_t)f * D.ccap + r] = has ? (int)(key & (MAX_TAB - 1)) : -1;
        D.connW[(size_t)f * D.ccap + r] = has ? (int)(key >> IDX_BITS) : 0;
    }
    if (threadIdx.x == 0) D.nConn[f] = cnt;
}

// ==== host side ==============================================================================================================================
bool csr_limits(const char *who, int n_tab, int cap, int n_pts, int n_obs_total) {
    if (!table_limits(who, n_tab, cap, n_pts)) return false;
    if (n_obs_total < 0) { set_error("%s: n_obs_total %d below 0", who, n_obs_total); return false; }
    return true;
}

const char *const WHO_REFRESH = "msl_refresh_map_points", *const WHO_COVIS = "msl_covisibility";

int check_refresh(int n_tab, int cap, int n_pts, int n_items, int n_obs_total, int what, const msl_refresh_params *params,
                  const msl_keypoint *kps_un, const uint8_t *desc, const int32_t *n_kps, const float *Tcw, const uint8_t *kf_flags,
                  const int32_t *obs_off, const int32_t *obs_kf, const int32_t *obs_idx, const float *pt_xyz, const uint8_t *pt_flags,
                  const int32_t *pt_ref, const int32_t *ids, msl_mem mem, uint8_t *out_desc, float *out_normal, float *out_dist, int32_t *best_obs,
                  int32_t *best_median, uint8_t *status, uint8_t *, float *, float *, msl_mem) {
    const char *who = WHO_REFRESH;
    if (what < 1 || what > (MSL_REFRESH_DESC | MSL_REFRESH_NORMAL)) { set_error("%s: what %d outside the mask MSL_REFRESH_DESC | MSL_REFRESH_NORMAL", who, what); return MSL_ERR_INVALID; }
    const bool wantN = what & MSL_REFRESH_NORMAL;
    if (!none_null(who, {MSL_NAMED(params), MSL_NAMED(desc), MSL_NAMED(n_kps), MSL_NAMED(kf_flags), MSL_NAMED(obs_off), MSL_NAMED(obs_kf),
                         MSL_NAMED(obs_idx), MSL_NAMED(pt_flags), MSL_NAMED(ids), MSL_NAMED(out_desc), MSL_NAMED(out_normal), MSL_NAMED(out_dist),
                         MSL_NAMED(best_obs), MSL_NAMED(best_median), MSL_NAMED(status)})) return MSL_ERR_INVALID;
    if (wantN && !none_null(who, {MSL_NAMED(kps_un), MSL_NAMED(Tcw), MSL_NAMED(pt_xyz), MSL_NAMED(pt_ref)})) return MSL_ERR_INVALID;
    if (!csr_limits(who, n_tab, cap, n_pts, n_obs_total)) return MSL_ERR_INVALID;
    if (n_items < 1 || n_items > n_pts) { set_error("%s: n_items %d outside 1 .. n_pts = %d", who, n_items, n_pts); return MSL_ERR_INVALID; }
    if (wantN && !levels_ok(who, params->nlevels)) return MSL_ERR_INVALID;
    char why[256];
    if (mem == MSL_MEM_HOST && (!check::csr_ok(n_tab, cap, n_pts, n_obs_total, obs_off, obs_kf, obs_idx, n_kps, why, sizeof(why)) ||
                                !check::items_ok("ids", n_pts, n_items, ids, true, why, sizeof(why)) ||
                                (wantN && !check::refs_ok(n_tab, n_items, ids, pt_ref, why, sizeof(why))))) return refuse(who, why);
    return MSL_OK;
}

int launch_refresh(msl_match *h, int n_tab, int cap, int n_pts, int n_items, int n_obs_total, int what, const msl_refresh_params *prm,
                   const msl_keypoint *kps_un, const uint8_t *desc, const int32_t *, const float *Tcw, const uint8_t *kf_flags,
                   const int32_t *obs_off, const int32_t *obs_kf, const int32_t *obs_idx, const float *pt_xyz, const uint8_t *pt_flags,
                   const int32_t *pt_ref, const int32_t *ids, msl_mem mem, uint8_t *out_desc, float *out_normal, float *out_dist, int32_t *best_obs,
                   int32_t *best_median, uint8_t *status, uint8_t *pt_desc, float *pt_normal, float *pt_dist, msl_mem out_mem) {
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    const bool wantD = what & MSL_REFRESH_DESC, wantN = what & MSL_REFRESH_NORMAL;
    const size_t T = (size_t)n_tab, nt = T * cap, F = (size_t)n_items, np = (size_t)n_pts, no = (size_t)n_obs_total;
    RefreshDev D{};
    D.nTab = n_tab; D.cap = cap; D.nPts = n_pts; D.nObs = n_obs_total; D.what = what;
    D.prm = *prm;
    Stage S(h, mem, out_mem);
    D.kps = S.in(wantN ? kps_un : nullptr, nt); D.desc = S.in(wantD ? desc : nullptr, 32 * nt); D.Tcw = S.in(wantN ? Tcw : nullptr, 12 * T);
    D.kfFlags = S.in(kf_flags, T);
    D.off = S.in(obs_off, np + 1); D.okf = S.in(no ? obs_kf : nullptr, no); D.oidx = S.in(no ? obs_idx : nullptr, no);
    D.xyz = S.in(wantN ? pt_xyz : nullptr, 3 * np); D.flags = S.in(pt_flags, np); D.ref = S.in(wantN ? pt_ref : nullptr, np); D.ids = S.in(ids, F);
    D.outDesc = S.out(out_desc, 32 * F); D.outNormal = S.out(out_normal, 3 * F); D.outDist = S.out(out_dist, 2 * F);
    D.bestObs = S.out(best_obs, F); D.bestMedian = S.out(best_median, F); D.status = S.out(status, F);
    D.ptDesc = S.inout(wantD ? pt_desc : nullptr, 32 * np); D.ptNormal = S.inout(wantN ? pt_normal : nullptr, 3 * np);
    D.ptDist = S.inout(wantN ? pt_dist : nullptr, 2 * np);
    MSL_HIP_TRY(S.error());
    hipLaunchKernelGGL(k_refresh, dim3((unsigned)n_items), dim3(WAVE), 0, h->stream, D);
    MSL_HIP_TRY(hipGetLastError());
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}

int check_covisibility(int n_tab, int cap, int n_pts, int n_items, int n_obs_total, int ccap, int, const int32_t *held_id, const int32_t *n_kps,
                       const uint8_t *pt_flags, const int32_t *obs_off, const int32_t *obs_kf, const int32_t *kf, msl_mem mem, int32_t *weight,
                       int32_t *conn, int32_t *conn_w, int32_t *n_conn, msl_mem) {
    const char *who = WHO_COVIS;
    if (!none_null(who, {MSL_NAMED(held_id), MSL_NAMED(n_kps), MSL_NAMED(pt_flags), MSL_NAMED(obs_off), MSL_NAMED(obs_kf), MSL_NAMED(kf),
                         MSL_NAMED(weight), MSL_NAMED(conn), MSL_NAMED(conn_w), MSL_NAMED(n_conn)})) return MSL_ERR_INVALID;
    if (!csr_limits(who, n_tab, cap, n_pts, n_obs_total)) return MSL_ERR_INVALID;
    if (n_items < 1 || n_items > n_tab) { set_error("%s: n_items %d outside 1 .. n_tab = %d", who, n_items, n_tab); return MSL_ERR_INVALID; }
    if (ccap < 1 || ccap > n_tab) { set_error("%s: ccap %d outside 1 .. n_tab = %d", who, ccap, n_tab); return MSL_ERR_INVALID; }
    char why[256];
    if (mem == MSL_MEM_HOST && (!check::csr_ok(n_tab, cap, n_pts, n_obs_total, obs_off, obs_kf, nullptr, n_kps, why, sizeof(why)) ||
                                !check::items_ok("kf", n_tab, n_items, kf, false, why, sizeof(why)))) return refuse(who, why);
    return MSL_OK;
}

int launch_covisibility(msl_match *h, int n_tab, int cap, int n_pts, int n_items, int n_obs_total, int ccap, int th, const int32_t *held_id,
                        const int32_t *n_kps, const uint8_t *pt_flags, const int32_t *obs_off, const int32_t *obs_kf, const int32_t *kf,
                        msl_mem mem, int32_t *weight, int32_t *conn, int32_t *conn_w, int32_t *n_conn, msl_mem out_mem) {
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    const size_t T = (size_t)n_tab, F = (size_t)n_items, np = (size_t)n_pts, no = (size_t)n_obs_total;
    CovisDev D{};
    D.nTab = n_tab; D.cap = cap; D.nPts = n_pts; D.nObs = n_obs_total; D.ccap = ccap; D.th = th; D.P = pow2_at_least(n_tab > 2 ? n_tab : 2);
    Stage S(h, mem, out_mem);
    D.held = S.in(held_id, T * cap); D.n = S.in(n_kps, T); D.flags = S.in(pt_flags, np);
    D.off = S.in(obs_off, np + 1); D.okf = S.in(no ? obs_kf : nullptr, no); D.kf = S.in(kf, F);
    D.weight = S.out(weight, F * T); D.conn = S.out(conn, F * ccap); D.connW = S.out(conn_w, F * ccap); D.nConn = S.out(n_conn, F);
    MSL_HIP_TRY(S.error());
    hipLaunchKernelGGL(k_covis, dim3((unsigned)n_items), dim3(COVIS_NT), 8 * (size_t)D.P + 4 * T, h->stream, D);   // at most 48 KB
    MSL_HIP_TRY(hipGetLastError());
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}

}  // namespace

extern "C" {

int msl_refresh_map_points(msl_match *h, int n_tab, int cap, int n_pts, int n_items, int n_obs_total, int what, const msl_refresh_params *params,
                           const msl_keypoint *kps_un, const uint8_t *desc, const int32_t *n_kps, const float *Tcw, const uint8_t *kf_flags,
                           const int32_t *obs_off, const int32_t *obs_kf, const int32_t *obs_idx, const float *pt_xyz, const uint8_t *pt_flags,
                           const int32_t *pt_ref, const int32_t *ids, msl_mem mem, uint8_t *out_desc, float *out_normal, float *out_dist,
                           int32_t *best_obs, int32_t *best_median, uint8_t *status, uint8_t *pt_desc, float *pt_normal, float *pt_dist,
                           msl_mem out_mem) noexcept {
    try {
    return handle_form(WHO_REFRESH, check_refresh, launch_refresh, h, n_tab, cap, n_pts, n_items, n_obs_total, what, params, kps_un, desc, n_kps, Tcw,
                       kf_flags, obs_off, obs_kf, obs_idx, pt_xyz, pt_flags, pt_ref, ids, mem, out_desc, out_normal, out_dist, best_obs, best_median,
                       status, pt_desc, pt_normal, pt_dist, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_refresh_map_points_batch(int device, int n_tab, int cap, int n_pts, int n_items, int n_obs_total, int what, const msl_refresh_params *params,
                                 const msl_keypoint *kps_un, const uint8_t *desc, const int32_t *n_kps, const float *Tcw, const uint8_t *kf_flags,
                                 const int32_t *obs_off, const int32_t *obs_kf, const int32_t *obs_idx, const float *pt_xyz,
                                 const uint8_t *pt_flags, const int32_t *pt_ref, const int32_t *ids, msl_mem mem, uint8_t *out_desc,
                                 float *out_normal, float *out_dist, int32_t *best_obs, int32_t *best_median, uint8_t *status, uint8_t *pt_desc,
                                 float *pt_normal, float *pt_dist, msl_mem out_mem) noexcept {
    try {
    return batch_form(check_refresh, launch_refresh, device, mem == MSL_MEM_DEVICE, n_tab, cap, n_pts, n_items, n_obs_total, what, params, kps_un,
                      desc, n_kps, Tcw, kf_flags, obs_off, obs_kf, obs_idx, pt_xyz, pt_flags, pt_ref, ids, mem, out_desc, out_normal, out_dist, best_obs,
                      best_median, status, pt_desc, pt_normal, pt_dist, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_covisibility(msl_match *h, int n_tab, int cap, int n_pts, int n_items, int n_obs_total, int ccap, int th, const int32_t *held_id,
                     const int32_t *n_kps, const uint8_t *pt_flags, const int32_t *obs_off, const int32_t *obs_kf, const int32_t *kf, msl_mem mem,
                     int32_t *weight, int32_t *conn, int32_t *conn_w, int32_t *n_conn, msl_mem out_mem) noexcept {
    try {
    return handle_form(WHO_COVIS, check_covisibility, launch_covisibility, h, n_tab, cap, n_pts, n_items, n_obs_total, ccap, th, held_id, n_kps,
                       pt_flags, obs_off, obs_kf, kf, mem, weight, conn, conn_w, n_conn, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_covisibility_batch(int device, int n_tab, int cap, int n_pts, int n_items, int n_obs_total, int ccap, int th, const int32_t *held_id,
                           const int32_t *n_kps, const uint8_t *pt_flags, const int32_t *obs_off, const int32_t *obs_kf, const int32_t *kf,
                           msl_mem mem, int32_t *weight, int32_t *conn, int32_t *conn_w, int32_t *n_conn, msl_mem out_mem) noexcept {
    try {
    return batch_form(check_covisibility, launch_covisibility, device, mem == MSL_MEM_DEVICE, n_tab, cap, n_pts, n_items, n_obs_total, ccap, th,
                      held_id, n_kps, pt_flags, obs_off, obs_kf, kf, mem, weight, conn, conn_w, n_conn, out_mem);
    } MSL_ABI_CATCH_INT
}

}  // extern "C"

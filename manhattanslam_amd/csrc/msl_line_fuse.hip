// msl_line_fuse.hip -- the line half of LocalMapping::SearchInNeighbors for gfx950 (reference src/LocalMapping.cc:583-618): LSDmatcher::Fuse
// (src/LSDmatcher.cpp:259-382) with KeyFrame::GetLinesInArea (src/KeyFrame.cc:506-538) and MapLine::PredictScale (src/MapLine.cpp:320-328) as
// msl_fuse_map_lines[_batch], MapLine::UpdateAverageDir (src/MapLine.cpp:262-308) as msl_refresh_map_lines[_batch].
//
// As for points (msl_fuse.hip) the search of one (target keyframe, map line) pair reads the keyframe's keylines and pose and the line's own
// position, normal, distance range and descriptor, never a slot and never another candidate; only the add / replace choice is ordered.
//   k_lfuse_query    one lane per (item, candidate): the exits of the loop body up to the radius, in order, into a 32-byte record
//   k_lfuse_search   one workgroup per (item, tile of 4 .. 64 candidates, sized so that a call has some 512 workgroups): the target's
//                    keylines (4 KB) and descriptors (8 KB) staged in LDS once; one wave per candidate, lane k testing keylines k,
//                    k + 64, ...: GetLinesInArea's two tests, the level window, the popcount distance; wave minimum of
//                    (dist << 8 | index) = the first minimum in ascending index
//   k_lfuse_resolve  one workgroup per item: held_id of the target in LDS; the first and the second matched j of every slot, the
//                    candidate that is the slot's own holder left out (a self-hit changes nothing), by two LDS atomicMin passes; then
//                    the slot walk of msl.h in closed form as in k_fuse_resolve, with membership of the added line read from the LDS
//                    held_id
//   k_line_refresh   one wave per line: the observations 64 at a time, the unit view vectors formed by the lanes in double and added in
//                    list order by shuffles, the same sum in every lane
// Pins (tests/linefuse_model.py is the sequential model; contraction off): the arithmetic of msl.h's lists; device-only: an id outside the
// line table is NULL, a tgt outside the keyframe table has no pose and no keylines, so its live candidates leave at the query as
// NO_FEATURE, a list outside the lists is empty.
#include "msl_fuse_list.h"
#include "msl_line_project.h"
#include "msl_index_check.h"
#include "msl_obs_walk.h"

#include <algorithm>
#include <climits>

namespace {

using namespace msl;

constexpr int QUERY_NT = 256, SEARCH_NT = 256, RESOLVE_NT = 1024;
constexpr int CODE_SEARCH = 255;                     // LfRec::code of a candidate that reaches GetLinesInArea

// The query of one (item, candidate), and what msl_debug_line_fuse reads
struct LfRec { float x1, y1, x2, y2, r; int32_t level, nidx, code; };

struct LfDev {
    int nTab, klcap, nLines, nItems, nLists, lcap, tile;   // tile: candidates per workgroup of k_lfuse_search
    msl_line_fuse_params prm;
    const msl_keyline *kl; const uint8_t *ldesc; const int32_t *nKl; const float *Tcw; const int32_t *held;
    const double *xyz, *normal; const float *dist; const uint8_t *desc, *flags; const int32_t *nobs;
    const int32_t *tgt, *list, *cand, *nCand;
    int32_t *bestIdx, *bestDist; uint8_t *status; int32_t *other, *nFused;
    LfRec *rec;
};

// ==== the loop body of LSDmatcher::Fuse up to the radius (:277-336) ===========================================================================
__global__ __launch_bounds__(QUERY_NT) void k_lfuse_query(LfDev D) {
    const int f = blockIdx.y, j = blockIdx.x * QUERY_NT + threadIdx.x;
    if (j >= D.lcap) return;
    const int32_t *row;
    const int nc = item_list(D, f, row);
    LfRec R{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0, 0, MSL_LFUSE_NULL};
    if (j < nc) {
        const int id = row[j], k = D.tgt[f];
        const msl_line_fuse_params &K = D.prm;
        do {
            if (id < 0 || id >= D.nLines) break;                               // :280 NULL
            R.code = MSL_LFUSE_BAD;
            if (!(D.flags[id] & 1)) break;                                     // :280 isBad()
            R.code = MSL_LFUSE_NO_FEATURE;
            if (k < 0 || k >= D.nTab) break;
            const float *T = D.Tcw + (size_t)k * 12;
            msl_match_params b{};
            b.fx = K.fx; b.fy = K.fy; b.cx = K.cx; b.cy = K.cy; b.minX = K.minX; b.maxX = K.maxX; b.minY = K.minY; b.maxY = K.maxY;
            float SP[3], EP[3];
            LineQ q{};
            if (!project_line(b, T, D.xyz + (size_t)id * 6, SP, EP, q)) {      // :283-317; which of its exits: the depths again
                const float tcw[3] = {T[3], T[7], T[11]};
                float SPc[3], EPc[3];
                gemm3(T, false, 1.0, SP, tcw, SPc);
                gemm3(T, false, 1.0, EP, tcw, EPc);
                R.code = (SPc[2] < 0.0f || EPc[2] < 0.0f) ? MSL_LFUSE_BEHIND : MSL_LFUSE_OUT_OF_IMAGE;
                break;
            }
            R.x1 = q.x1; R.y1 = q.y1; R.x2 = q.x2; R.y2 = q.y2;
            const float dmin = D.dist[2 * (size_t)id], dmax = D.dist[2 * (size_t)id + 1];
            const float maxDistance = 1.2f * dmax, minDistance = 0.8f * dmin;  // :319-320
            float Ow[3];
            camera_centre(T, Ow);
            float OM[3];
            for (int a = 0; a < 3; a++) OM[a] = (SP[a] * 0.5f + EP[a] * 0.5f + 0.0f) - Ow[a];   // :322, as msl_line_match.hip's local_query
            double ss = 0.0;
            for (int a = 0; a < 3; a++) ss += (double)OM[a] * (double)OM[a];
            const float dist = (float)sqrt(ss);                                // :323 cv::norm
            R.code = MSL_LFUSE_DISTANCE;
            if (dist < minDistance || dist > maxDistance) break;               // :325
            const double *Pn = D.normal + (size_t)id * 3;
            double dot = 0.0;
            for (int a = 0; a < 3; a++) dot += (double)OM[a] * (double)(float)Pn[a];             // :329-331
            R.code = MSL_LFUSE_VIEW_ANGLE;
            if (dot < 0.5 * (double)dist) break;
            const int L = predict_level(dmax, dist, K.log_scale_factor);       // :334, not clamped
            R.level = L;
            R.r = K.th * K.scale_factors[clampi(L, 0, K.nlevels - 1)];         // :336 (level clamped for the lookup only)
            R.code = CODE_SEARCH;
        } while (false);
    }
    D.rec[(size_t)f * D.lcap + j] = R;
}

// ==== GetLinesInArea and the candidate loop (:338-362) ========================================================================================
__global__ __launch_bounds__(SEARCH_NT) void k_lfuse_search(LfDev D) {
    __shared__ msl_keyline s_kl[MAX_KLCAP];
    __shared__ uint4 s_desc[2 * MAX_KLCAP];
    const int f = blockIdx.y, j0 = blockIdx.x * D.tile, lane = lane_id(), w = threadIdx.x >> 6;
    const int32_t *row;
    const int nc = item_list(D, f, row);
    const int k = D.tgt[f];
    int nkl = 0;
    if (j0 < nc && k >= 0 && k < D.nTab) {                                     // uniform per workgroup
        nkl = clampi(D.nKl[k], 0, D.klcap);
        const size_t kb = (size_t)k * D.klcap;
        for (int i = threadIdx.x; i < nkl; i += SEARCH_NT) {
            s_kl[i] = D.kl[kb + i];
            load_desc(D.ldesc + (kb + i) * 32, s_desc[2 * i], s_desc[2 * i + 1]);
        }
    }
    __syncthreads();
    const int jEnd = min(j0 + D.tile, D.lcap);
    for (int j = j0 + w; j < jEnd; j += SEARCH_NT / WAVE) {                    // one wave per candidate; everything but the keyline loop uniform
        const size_t o = (size_t)f * D.lcap + j;
        const LfRec R = D.rec[o];
        int status = R.code, bestIdx = -1, bestDist = j < nc ? INT_MAX : 0, cnt = 0;
        if (R.code == CODE_SEARCH) {
            uint4 d0, d1;
            load_desc(D.desc + (size_t)row[j] * 32, d0, d1);
            const double mx = 0.5 * (double)(R.x1 + R.x2), my = 0.5 * (double)(R.y1 + R.y2);   // float sums, then double
            const float slope0 = (R.y1 - R.y2) / (R.x1 - R.x2);
            const float rr = R.r * R.r;
            const double rs = (double)R.r * 0.01;
            const int Lm1 = wrap_add(R.level, -1);
            unsigned key = NO_ENTRY;
            for (int i = lane; i < nkl; i += WAVE) {
                const msl_keyline kl = s_kl[i];
                const double dx = mx - (double)kl.x, dy = my - (double)kl.y;
                const float distance = (float)(dx * dx + dy * dy);
                if (distance > rr) continue;
                const float slope = slope0 - kl.angle;                         // no fabs: a negative difference, or NaN, passes
                if ((double)slope > rs) continue;
                cnt++;
                if (kl.octave < Lm1 || kl.octave > R.level) continue;          // :351
                const unsigned dist = (unsigned)hamming256(d0, d1, s_desc[2 * i], s_desc[2 * i + 1]);
                const unsigned kk = (dist << 8) | (unsigned)i;
                key = kk < key ? kk : key;
            }
            key = wave_min(key);
            cnt = wave_sum(cnt);
            if (cnt == 0) status = MSL_LFUSE_NO_FEATURE;                       // :340
            else if (key == NO_ENTRY) status = MSL_LFUSE_NO_CANDIDATE;
            else {
                bestDist = (int)(key >> 8); bestIdx = (int)(key & 255u);
                status = bestDist <= D.prm.th_low ? MSL_LFUSE_ADDED : MSL_LFUSE_ABOVE_TH_LOW;   // ADDED: matched; k_lfuse_resolve decides
            }
        }
        if (lane == 0) {
            D.bestIdx[o] = bestIdx; D.bestDist[o] = bestDist; D.status[o] = (uint8_t)status; D.other[o] = -1;
            if (R.code == CODE_SEARCH) D.rec[o].nidx = cnt;
        }
    }
}

// ==== the slot walk ==========================================================================================================================
__global__ __launch_bounds__(RESOLVE_NT) void k_lfuse_resolve(LfDev D) {
    __shared__ int s_held[MAX_KLCAP];                                          // the live-table holder of every slot, -1 for none
    __shared__ unsigned s_first[MAX_KLCAP], s_second[MAX_KLCAP];               // first / second matched j that is not the slot's own holder
    __shared__ int s_hold[MAX_KLCAP];                                          // the holder after the slot's deciding hit
    __shared__ unsigned s_keeps[MAX_KLCAP];
    __shared__ unsigned s_count;
    const int f = blockIdx.x;
    const int32_t *row;
    const int nc = item_list(D, f, row);
    const int k = D.tgt[f];
    const int nkl = (k >= 0 && k < D.nTab) ? clampi(D.nKl[k], 0, D.klcap) : 0;
    const size_t fb = (size_t)f * D.lcap;
    for (int s = threadIdx.x; s < MAX_KLCAP; s += RESOLVE_NT) {
        int h = -1;
        if (s < nkl) { h = D.held[(size_t)k * D.klcap + s]; if (h < 0 || h >= D.nLines) h = -1; }
        s_held[s] = h; s_first[s] = NO_ENTRY; s_second[s] = NO_ENTRY; s_hold[s] = -1; s_keeps[s] = 0;
    }
    if (threadIdx.x == 0) s_count = 0;
    __syncthreads();
    first_two_hits<RESOLVE_NT>(D.status, D.bestIdx, fb, MSL_LFUSE_ADDED, nc, s_first, s_second,
                               [&](int j, int s) { return row[j] == s_held[s]; });   // a self-hit changes nothing
    for (int s = threadIdx.x; s < nkl; s += RESOLVE_NT) {                      // the holder and the direction after the deciding hit
        const unsigned j1 = s_first[s], j2 = s_second[s];
        if (j1 == NO_ENTRY) continue;
        const int h0 = s_held[s], p1 = row[j1];
        if (h0 >= 0) {
            const bool keeps = D.nobs[h0] > D.nobs[p1];
            s_keeps[s] = keeps; s_hold[s] = keeps ? h0 : p1;
        } else if (j2 != NO_ENTRY) {
            const int p2 = row[j2];
            bool in = false;                                                   // AddObservation's early return: p1 is in the keyframe already
            for (int t = 0; t < nkl; t++) in = in || s_held[t] == p1;
            const bool keeps = D.nobs[p1] + (in ? 0 : 1) > D.nobs[p2];
            s_keeps[s] = keeps; s_hold[s] = keeps ? p1 : p2;
        }
    }
    __syncthreads();
    int mine = 0;
    for (int j = threadIdx.x; j < nc; j += RESOLVE_NT) {
        if (D.status[fb + j] != MSL_LFUSE_ADDED) continue;                     // a matched candidate: its tgt is a table keyframe
        mine++;
        const int s = D.bestIdx[fb + j], p = row[j], h0 = s_held[s];
        const unsigned j1 = s_first[s], j2 = s_second[s];
        const bool keeps = s_keeps[s];
        int st, oth;
        if (h0 >= 0 && !(D.flags[h0] & 1)) { st = MSL_LFUSE_HELD_BAD; oth = h0; }
        else if (p == h0) {
            if ((unsigned)j < j1) { st = MSL_LFUSE_SELF; oth = h0; }
            else { st = MSL_LFUSE_UNRESOLVED; oth = s_hold[s]; }
        } else if (h0 < 0) {
            if ((unsigned)j == j1) { st = MSL_LFUSE_ADDED; oth = -1; }
            else if ((unsigned)j == j2) { st = keeps ? MSL_LFUSE_REPLACED_BY_HELD : MSL_LFUSE_REPLACES_HELD; oth = row[j1]; }
            else { st = MSL_LFUSE_UNRESOLVED; oth = s_hold[s]; }
        } else {
            if ((unsigned)j == j1) { st = keeps ? MSL_LFUSE_REPLACED_BY_HELD : MSL_LFUSE_REPLACES_HELD; oth = h0; }
            else { st = MSL_LFUSE_UNRESOLVED; oth = s_hold[s]; }
        }
        D.status[fb + j] = (uint8_t)st; D.other[fb + j] = oth;
    }
    mine = wave_sum(mine);
    if (lane_id() == 0 && mine) atomicAdd(&s_count, (unsigned)mine);
    __syncthreads();
    if (threadIdx.x == 0) D.nFused[f] = (int)s_count;
}

// ==== MapLine::UpdateAverageDir of one line ==================================================================================================
struct LrDev {
    int nTab, klcap, nLines, nObs;
    msl_refresh_params prm;
    const msl_keyline *kl; const float *Tcw;
    const int32_t *off, *okf, *oidx;
    const double *xyz; const uint8_t *flags; const int32_t *ref, *ids;
    double *outNormal; float *outDist; uint8_t *status;
    double *lnNormal; float *lnDist;
};

__global__ __launch_bounds__(WAVE) void k_line_refresh(LrDev D) {
    const int f = blockIdx.x, lane = threadIdx.x;
    const int id = D.ids[f];
    int status = MSL_REFRESH_BAD;
    double normal[3] = {0.0, 0.0, 0.0};
    float dist[2] = {0.0f, 0.0f};
    if (id >= 0 && id < D.nLines && (D.flags[id] & 1)) {                       // uniform, as every branch outside the lane loops
        int b, e;
        obs_range(D, id, b, e);
        const int ref = D.ref[id];
        const double *P = D.xyz + (size_t)id * 6;
        double mid[3];
#pragma unroll
        for (int a = 0; a < 3; a++) mid[a] = 0.5 * (P[a] + P[3 + a]);          // :286 middlePos
        int n = 0, refIdx = 0;                                                 // refIdx 0: map::operator[] of an absent key
        bool refSeen = false;
        double acc[3] = {0.0, 0.0, 0.0};
        for (int c = b; c < e; c += WAVE) {
            int kk, idx;
            bool valid;
            const unsigned long long m = obs_chunk(D, c + lane, e, kk, idx, valid);
            n += __popcll(m);
            double t[3] = {0.0, 0.0, 0.0};
            if (valid) {
                float Ow[3];
                camera_centre(D.Tcw + (size_t)kk * 12, Ow);
                double v[3];
#pragma unroll
                for (int a = 0; a < 3; a++) v[a] = mid[a] - (double)Ow[a];     // :287
                const double nrm = sqrt(v[0] * v[0] + (v[1] * v[1] + v[2] * v[2]));   // Eigen's unrolled 3-vector reduction
#pragma unroll
                for (int a = 0; a < 3; a++) t[a] = v[a] / nrm;
            }
            obs_ref_index(valid && kk == ref, idx, refSeen, refIdx);
            obs_add_in_order(m, t, acc);                                       // normal = normal + normali / norm, in list order
        }
        status = MSL_REFRESH_NO_OBS;
        if (n > 0) {
            int level = -1;
            if (ref >= 0 && ref < D.nTab && refIdx >= 0 && refIdx < D.klcap) level = D.kl[(size_t)ref * D.klcap + refIdx].octave;
            if (level < 0 || level >= D.prm.nlevels) status = MSL_REFRESH_BAD_OCTAVE;
            else {
                float Ow[3], CM[3];
                camera_centre(D.Tcw + (size_t)ref * 12, Ow);
#pragma unroll
                for (int a = 0; a < 3; a++) CM[a] = ((float)P[a] * 0.5f + (float)P[3 + a] * 0.5f + 0.0f) - Ow[a];   // :292-296
                const float d = (float)norm3_dacc(CM);                         // :297
                dist[1] = d * D.prm.scale_factors[level];                      // :304
                dist[0] = dist[1] / D.prm.scale_factors[D.prm.nlevels - 1];    // :305
                const double dn = (double)n;
#pragma unroll
                for (int a = 0; a < 3; a++) normal[a] = acc[a] / dn;           // :306
                status = MSL_REFRESH_NORMAL_WRITTEN;
            }
        }
    }
    if (lane == 0) {
        D.status[f] = (uint8_t)status;
        const bool wrote = status == MSL_REFRESH_NORMAL_WRITTEN;
        write_item_and_row(D.outNormal, D.lnNormal, wrote, f, id, normal);
        write_item_and_row(D.outDist, D.lnDist, wrote, f, id, dist);
    }
}

// ==== host side ==============================================================================================================================
const char *const WHO_LFUSE = "msl_fuse_map_lines", *const WHO_LREFRESH = "msl_refresh_map_lines";

int check_line_fuse(int n_tab, int klcap, int n_lines, int n_items, int n_lists, int lcap, const msl_line_fuse_params *params, const msl_keyline *kl,
                    const uint8_t *ldesc, const int32_t *n_kl, const float *Tcw, const int32_t *held_id, const double *ln_xyz,
                    const double *ln_normal, const float *ln_dist, const uint8_t *ln_desc, const uint8_t *ln_flags, const int32_t *ln_nobs,
                    const int32_t *tgt, const int32_t *list, const int32_t *cand, const int32_t *n_cand, msl_mem mem, int32_t *best_idx,
                    int32_t *best_dist, uint8_t *status, int32_t *other, int32_t *n_fused, msl_mem) {
    const char *who = WHO_LFUSE;
    if (!none_null(who, {MSL_NAMED(params), MSL_NAMED(kl), MSL_NAMED(ldesc), MSL_NAMED(n_kl), MSL_NAMED(Tcw), MSL_NAMED(held_id), MSL_NAMED(ln_xyz),
                         MSL_NAMED(ln_normal), MSL_NAMED(ln_dist), MSL_NAMED(ln_desc), MSL_NAMED(ln_flags), MSL_NAMED(ln_nobs), MSL_NAMED(tgt),
                         MSL_NAMED(list), MSL_NAMED(cand), MSL_NAMED(n_cand), MSL_NAMED(best_idx), MSL_NAMED(best_dist), MSL_NAMED(status),
                         MSL_NAMED(other), MSL_NAMED(n_fused)})) return MSL_ERR_INVALID;
    if (!line_table_limits(who, n_tab, klcap, n_lines) || !item_limits(who, n_items, lcap)) return MSL_ERR_INVALID;
    if (n_lists < 1) { set_error("%s: n_lists %d below 1", who, n_lists); return MSL_ERR_INVALID; }
    if (!levels_ok(who, params->nlevels)) return MSL_ERR_INVALID;
    if (params->th_low < 0 || params->th_low > 256) { set_error("%s: th_low %d outside 0 .. 256", who, params->th_low); return MSL_ERR_INVALID; }
    char why[256];
    if (mem == MSL_MEM_HOST && !check::lists_ok("line", n_tab, n_lines, n_items, n_lists, lcap, tgt, list, cand, n_cand, why, sizeof(why))) return refuse(who, why);
    return MSL_OK;
}

int launch_line_fuse(msl_match *h, int n_tab, int klcap, int n_lines, int n_items, int n_lists, int lcap, const msl_line_fuse_params *prm,
                     const msl_keyline *kl, const uint8_t *ldesc, const int32_t *n_kl, const float *Tcw, const int32_t *held_id, const double *ln_xyz,
                     const double *ln_normal, const float *ln_dist, const uint8_t *ln_desc, const uint8_t *ln_flags, const int32_t *ln_nobs,
                     const int32_t *tgt, const int32_t *list, const int32_t *cand, const int32_t *n_cand, msl_mem mem, int32_t *best_idx,
                     int32_t *best_dist, uint8_t *status, int32_t *other, int32_t *n_fused, msl_mem out_mem) {
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    hipStream_t st = h->stream;
    const size_t T = (size_t)n_tab, nt = T * klcap, F = (size_t)n_items, L = (size_t)n_lists, nl = (size_t)n_lines, nf = F * lcap;
    LfDev D{};
    D.nTab = n_tab; D.klcap = klcap; D.nLines = n_lines; D.nItems = n_items; D.nLists = n_lists; D.lcap = lcap;
    D.tile = std::min(std::max(pow2_at_least((int)((nf + 511) / 512)), SEARCH_NT / WAVE), 64);
    D.prm = *prm;
    MSL_HIP_TRY(grow_all(st, {{h->lfuseRec, sizeof(LfRec) * nf}}));
    h->lfuseItems = n_items; h->lfuseLcap = lcap;
    Stage S(h, mem, out_mem);
    D.kl = S.in(kl, nt); D.ldesc = S.in(ldesc, 32 * nt); D.nKl = S.in(n_kl, T); D.Tcw = S.in(Tcw, 12 * T); D.held = S.in(held_id, nt);
    D.xyz = S.in(ln_xyz, 6 * nl); D.normal = S.in(ln_normal, 3 * nl); D.dist = S.in(ln_dist, 2 * nl); D.desc = S.in(ln_desc, 32 * nl);
    D.flags = S.in(ln_flags, nl); D.nobs = S.in(ln_nobs, nl);
    D.tgt = S.in(tgt, F); D.list = S.in(list, F); D.cand = S.in(cand, L * lcap); D.nCand = S.in(n_cand, L);
    D.bestIdx = S.out(best_idx, nf); D.bestDist = S.out(best_dist, nf); D.status = S.out(status, nf); D.other = S.out(other, nf);
    D.nFused = S.out(n_fused, F);
    MSL_HIP_TRY(S.error());
    D.rec = (LfRec *)h->lfuseRec.p;
    hipLaunchKernelGGL(k_lfuse_query, dim3((unsigned)((lcap + QUERY_NT - 1) / QUERY_NT), (unsigned)n_items), dim3(QUERY_NT), 0, st, D);
    MSL_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_lfuse_search, dim3((unsigned)((lcap + D.tile - 1) / D.tile), (unsigned)n_items), dim3(SEARCH_NT), 0, st, D);
    MSL_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_lfuse_resolve, dim3((unsigned)n_items), dim3(RESOLVE_NT), 0, st, D);
    MSL_HIP_TRY(hipGetLastError());
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}

int check_line_refresh(int n_tab, int klcap, int n_lines, int n_items, int n_obs_total, const msl_refresh_params *params, const msl_keyline *kl,
                       const int32_t *n_kl, const float *Tcw, const int32_t *obs_off, const int32_t *obs_kf, const int32_t *obs_idx,
                       const double *ln_xyz, const uint8_t *ln_flags, const int32_t *ln_ref, const int32_t *ids, msl_mem mem, double *out_normal,
                       float *out_dist, uint8_t *status, double *, float *, msl_mem) {
    const char *who = WHO_LREFRESH;
    if (!none_null(who, {MSL_NAMED(params), MSL_NAMED(kl), MSL_NAMED(n_kl), MSL_NAMED(Tcw), MSL_NAMED(obs_off), MSL_NAMED(obs_kf), MSL_NAMED(obs_idx),
                         MSL_NAMED(ln_xyz), MSL_NAMED(ln_flags), MSL_NAMED(ln_ref), MSL_NAMED(ids), MSL_NAMED(out_normal), MSL_NAMED(out_dist),
                         MSL_NAMED(status)})) return MSL_ERR_INVALID;
    if (!line_table_limits(who, n_tab, klcap, n_lines)) return MSL_ERR_INVALID;
    if (n_obs_total < 0) { set_error("%s: n_obs_total %d below 0", who, n_obs_total); return MSL_ERR_INVALID; }
    if (n_items < 1 || n_items > n_lines) { set_error("%s: n_items %d outside 1 .. n_lines = %d", who, n_items, n_lines); return MSL_ERR_INVALID; }
    if (!levels_ok(who, params->nlevels)) return MSL_ERR_INVALID;
    char why[256];
    if (mem == MSL_MEM_HOST && (!check::csr_ok(n_tab, klcap, n_lines, n_obs_total, obs_off, obs_kf, obs_idx, n_kl, why, sizeof(why)) ||
                                !check::items_ok("ids", n_lines, n_items, ids, true, why, sizeof(why)))) return refuse(who, why);
    return MSL_OK;
}

int launch_line_refresh(msl_match *h, int n_tab, int klcap, int n_lines, int n_items, int n_obs_total, const msl_refresh_params *prm,
                        const msl_keyline *kl, const int32_t *, const float *Tcw, const int32_t *obs_off, const int32_t *obs_kf,
                        const int32_t *obs_idx, const double *ln_xyz, const uint8_t *ln_flags, const int32_t *ln_ref, const int32_t *ids, msl_mem mem,
                        double *out_normal, float *out_dist, uint8_t *status, double *ln_normal, float *ln_dist, msl_mem out_mem) {
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    const size_t T = (size_t)n_tab, nt = T * klcap, F = (size_t)n_items, nl = (size_t)n_lines, no = (size_t)n_obs_total;
    LrDev D{};
    D.nTab = n_tab; D.klcap = klcap; D.nLines = n_lines; D.nObs = n_obs_total;
    D.prm = *prm;
    Stage S(h, mem, out_mem);
    D.kl = S.in(kl, nt); D.Tcw = S.in(Tcw, 12 * T);
    D.off = S.in(obs_off, nl + 1); D.okf = S.in(no ? obs_kf : nullptr, no); D.oidx = S.in(no ? obs_idx : nullptr, no);
    D.xyz = S.in(ln_xyz, 6 * nl); D.flags = S.in(ln_flags, nl); D.ref = S.in(ln_ref, nl); D.ids = S.in(ids, F);
    D.outNormal = S.out(out_normal, 3 * F); D.outDist = S.out(out_dist, 2 * F); D.status = S.out(status, F);
    D.lnNormal = S.inout(ln_normal, 3 * nl); D.lnDist = S.inout(ln_dist, 2 * nl);
    MSL_HIP_TRY(S.error());
    hipLaunchKernelGGL(k_line_refresh, dim3((unsigned)n_items), dim3(WAVE), 0, h->stream, D);
    MSL_HIP_TRY(hipGetLastError());
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}

}  // namespace

extern "C" {

int msl_fuse_map_lines(msl_match *h, int n_tab, int klcap, int n_lines, int n_items, int n_lists, int lcap, const msl_line_fuse_params *params,
                       const msl_keyline *kl, const uint8_t *ldesc, const int32_t *n_kl, const float *Tcw, const int32_t *held_id,
                       const double *ln_xyz, const double *ln_normal, const float *ln_dist, const uint8_t *ln_desc, const uint8_t *ln_flags,
                       const int32_t *ln_nobs, const int32_t *tgt, const int32_t *list, const int32_t *cand, const int32_t *n_cand, msl_mem mem,
                       int32_t *best_idx, int32_t *best_dist, uint8_t *status, int32_t *other, int32_t *n_fused, msl_mem out_mem) noexcept {
    try {
    return handle_form(WHO_LFUSE, check_line_fuse, launch_line_fuse, h, n_tab, klcap, n_lines, n_items, n_lists, lcap, params, kl, ldesc, n_kl, Tcw,
                       held_id, ln_xyz, ln_normal, ln_dist, ln_desc, ln_flags, ln_nobs, tgt, list, cand, n_cand, mem, best_idx, best_dist, status, other,
                       n_fused, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_fuse_map_lines_batch(int device, int n_tab, int klcap, int n_lines, int n_items, int n_lists, int lcap, const msl_line_fuse_params *params,
                             const msl_keyline *kl, const uint8_t *ldesc, const int32_t *n_kl, const float *Tcw, const int32_t *held_id,
                             const double *ln_xyz, const double *ln_normal, const float *ln_dist, const uint8_t *ln_desc, const uint8_t *ln_flags,
                             const int32_t *ln_nobs, const int32_t *tgt, const int32_t *list, const int32_t *cand, const int32_t *n_cand,
                             msl_mem mem, int32_t *best_idx, int32_t *best_dist, uint8_t *status, int32_t *other, int32_t *n_fused,
                             msl_mem out_mem) noexcept {
    try {
    return batch_form(check_line_fuse, launch_line_fuse, device, mem == MSL_MEM_DEVICE, n_tab, klcap, n_lines, n_items, n_lists, lcap, params, kl,
                      ldesc, n_kl, Tcw, held_id, ln_xyz, ln_normal, ln_dist, ln_desc, ln_flags, ln_nobs, tgt, list, cand, n_cand, mem, best_idx, best_dist,
                      status, other, n_fused, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_refresh_map_lines(msl_match *h, int n_tab, int klcap, int n_lines, int n_items, int n_obs_total, const msl_refresh_params *params,
                          const msl_keyline *kl, const int32_t *n_kl, const float *Tcw, const int32_t *obs_off, const int32_t *obs_kf,
                          const int32_t *obs_idx, const double *ln_xyz, const uint8_t *ln_flags, const int32_t *ln_ref, const int32_t *ids,
                          msl_mem mem, double *out_normal, float *out_dist, uint8_t *status, double *ln_normal, float *ln_dist,
                          msl_mem out_mem) noexcept {
    try {
    return handle_form(WHO_LREFRESH, check_line_refresh, launch_line_refresh, h, n_tab, klcap, n_lines, n_items, n_obs_total, params, kl, n_kl, Tcw,
                       obs_off, obs_kf, obs_idx, ln_xyz, ln_flags, ln_ref, ids, mem, out_normal, out_dist, status, ln_normal, ln_dist, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_refresh_map_lines_batch(int device, int n_tab, int klcap, int n_lines, int n_items, int n_obs_total, const msl_refresh_params *params,
                                const msl_keyline *kl, const int32_t *n_kl, const float *Tcw, const int32_t *obs_off, const int32_t *obs_kf,
                                const int32_t *obs_idx, const double *ln_xyz, const uint8_t *ln_flags, const int32_t *ln_ref, const int32_t *ids,
                                msl_mem mem, double *out_normal, float *out_dist, uint8_t *status, double *ln_normal, float *ln_dist,
                                msl_mem out_mem) noexcept {
    try {
    return batch_form(check_line_refresh, launch_line_refresh, device, mem == MSL_MEM_DEVICE || ((ln_normal || ln_dist) && out_mem == MSL_MEM_DEVICE),
                      n_tab, klcap, n_lines, n_items, n_obs_total, params, kl, n_kl, Tcw, obs_off, obs_kf, obs_idx, ln_xyz, ln_flags, ln_ref, ids, mem,
                      out_normal, out_dist, status, ln_normal, ln_dist, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_debug_line_fuse(msl_match *h, int item, float *uvr, int32_t *level_n) noexcept {
    try {
    if (!h || !uvr || !level_n || item < 0 || item >= h->lfuseItems || !h->lfuseRec.p) {
        set_error("msl_debug_line_fuse: invalid argument (item outside the last msl_fuse_map_lines call?)");
        return MSL_ERR_INVALID;
    }
    std::vector<LfRec> rec;
    int rc = last_call_row(h, h->lfuseRec, (size_t)item, (size_t)h->lfuseLcap, rec);
    if (rc != MSL_OK) return rc;
    for (int j = 0; j < h->lfuseLcap; j++) {
        const LfRec &r = rec[(size_t)j];
        uvr[5 * j] = r.x1; uvr[5 * j + 1] = r.y1; uvr[5 * j + 2] = r.x2; uvr[5 * j + 3] = r.y2; uvr[5 * j + 4] = r.r;
        level_n[2 * j] = r.level; level_n[2 * j + 1] = r.nidx;
    }
    return MSL_OK;
    } MSL_ABI_CATCH_INT
}

}  // extern "C"

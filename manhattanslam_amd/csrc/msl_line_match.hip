// msl_line_match.hip -- batched map-line matching by projection for gfx950: both overloads of LSDmatcher::SearchByProjection.
//
// msl_match_lines_by_projection  LSDmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th)  (reference src/LSDmatcher.cpp:21-134)
// msl_match_local_lines          Tracking::SearchLocalLines after its first loop (src/Tracking.cc:1697-1737): Frame::isInFrustum(MapLine*)
//                                (src/Frame.cc:261-327) + MapLine::PredictScale (src/MapLine.cpp:320-328), then
//                                LSDmatcher::SearchByProjection(Frame &F, const vector<MapLine*> &, th)  (src/LSDmatcher.cpp:137-198)
// both with Frame::GetLinesInArea (src/Frame.cc:384-415), a brute-force scan over the frame's keylines (no grid).
//
// Frame batched, two launches per call; the two searches share the candidate test and the assignment and differ in their query:
//   k_line_query   one lane per line (last-frame line or local map line): the window of the line -- projected endpoints, radius, octave range --
//                  stored as a LineQ.  last_query: the endpoint projection, th * mvScaleFactors[nLastOctave], the forward / backward / both-ways
//                  octave range of the frame pair (search_mode).  local_query: isInFrustum (writes mbTrackInView and the track record), then
//                  RadiusByViewingCos * th * mvScaleFactors[level], octaves [level - 1, level].
//   k_line_assign  one workgroup per frame: the frame's keylines (16 B) and descriptors (32 B) staged once in LDS (12 KB at lcap = 256); every
//                  line scans them against its window (GetLinesInArea) and the reference's greedy hand-out is solved as the min-fixpoint of
//                  msl_assign.h; then nToMatch and the pose-layout line_xyz / line_has.
// Arithmetic follows the reference's float / double mix literally (DESIGN.md section 3 lists the pins); gemm3, search_mode, hamming256 and
// predict_level are the point matcher's (msl_match_math.h).  The optional line_xyz / line_has arrays are in/out (untouched slots keep
// their bytes): staged from host memory like inputs, and a reason for the _batch forms to wait for the legacy stream.
#include "msl_assign.h"
#include "msl_line_project.h"
#include "msl_match_handle.h"

#include <climits>
#include <mutex>

using namespace msl;

namespace {

constexpr int TH_HIGH = 100;                       // src/LSDmatcher.cpp:15
constexpr int MAX_LLCAP = 256;                     // lines of the last frame; keylines: MAX_KLCAP, local map lines: MAX_MCAP (msl_match_handle.h)
constexpr int LINE_NT = 1024;
constexpr unsigned K_NONE = 0xFFFFFFFFu;

struct LineDev {
    int lcap, ncap;                                 // keylines per frame; lines per frame (llcap or mlcap)
    msl_line_match_params prm;
    float mb;                                       // mbf / fx (last-frame search)
    const msl_keyline *curKl; const uint8_t *curDesc; const int32_t *nCur; const uint8_t *curFlags;   // curFlags: local search only
    const double *xyz; const uint8_t *desc, *flags; const int32_t *nLines;                          // the lines (last frame or local map)
    const int32_t *octave;                                                                           // last-frame search only
    const double *normal; const float *dist;                                                         // local search only
    const float *TcwCur, *TcwLast;
    LineQ *q;                                       // [n][ncap] scratch written by k_line_query
    uint8_t *inView; msl_line_track *track;         // [n][mlcap] scratch (local search)
    uint8_t *inViewOut; msl_line_track *trackOut;   // the caller's device arrays (or nullptr)
    int32_t *matchOut, *nmatches, *nToMatch;
    double *lineXyz; uint8_t *lineHas;              // optional, [n][lcap] in msl_pose_optimize's layout
};

// last-frame line i (src/LSDmatcher.cpp:37-91)
__device__ __forceinline__ bool last_query(const LineDev &D, int f, int i, LineQ &q) {
    const size_t ii = (size_t)f * D.ncap + i;
    if (!(D.flags[ii] & 1)) return false;                                   // :40 NULL, bad or an outlier
    const float *Tc = D.TcwCur + (size_t)f * 12;
    float SP[3], EP[3];
    if (!project_line(D.prm.base, Tc, D.xyz + ii * 6, SP, EP, q)) return false;
    const int o = D.octave[ii];
    q.r = D.prm.base.th * D.prm.base.scale_factors[clampi(o, 0, D.prm.base.nlevels - 1)];   // :82 (octave clamped for the lookup)
    const int mode = search_mode(Tc, D.TcwLast + (size_t)f * 12, D.mb);
    if (mode == 1) { q.minLevel = o; q.maxLevel = -1; }                     // :86-91, GetLinesInArea's default maxLevel = -1
    else if (mode == 2) { q.minLevel = 0; q.maxLevel = o; }
    else { q.minLevel = wrap_add(o, -1); q.maxLevel = wrap_add(o, 1); }
    return true;
}

// local map line i: isInFrustum (src/Frame.cc:261-327) -> mbTrackInView + track, then the window of src/LSDmatcher.cpp:143-157
__device__ __forceinline__ bool local_query(const LineDev &D, int f, int i, LineQ &q, msl_line_track &t) {
    const size_t ii = (size_t)f * D.ncap + i;
    if (!(D.flags[ii] & 1)) return false;                                   // SearchLocalLines: seen in this frame, or bad
    const msl_match_params &b = D.prm.base;
    const float *Tc = D.TcwCur + (size_t)f * 12;
    float SP[3], EP[3];
    if (!project_line(b, Tc, D.xyz + ii * 6, SP, EP, q)) return false;
    const float dmin = D.dist[2 * ii], dmax = D.dist[2 * ii + 1];
    const float maxDistance = 1.2f * dmax, minDistance = 0.8f * dmin;     // GetMax / GetMinDistanceInvariance (src/MapLine.cpp:310-318)
    const float tcw[3] = {Tc[3], Tc[7], Tc[11]};
    float Ow[3];
    gemm3(Tc, true, -1.0, tcw, nullptr, Ow);                                // mOw = -mRcw.t() * mtcw
    float OM[3];
    for (int k = 0; k < 3; k++) OM[k] = (SP[k] * 0.5f + EP[k] * 0.5f + 0.0f) - Ow[k];   // :302 addWeighted(SP, .5, EP, .5, 0) - mOw, float
    double ss = 0.0;
    for (int k = 0; k < 3; k++) ss += (double)OM[k] * (double)OM[k];
    const float dist = (float)sqrt(ss);                                     // :303 cv::norm
    if (dist < minDistance || dist > maxDistance) return false;             // :305
    const double *Pn = D.normal + ii * 3;
    double dot = 0.0;
    for (int k = 0; k < 3; k++) dot += (double)OM[k] * (double)(float)Pn[k];   // :309-310 Mat_<float> normal, Mat::dot in double
    const float viewCos = (float)(dot / (double)dist);
    if (viewCos < D.prm.view_cos_limit) return false;                       // :312
    const int L = predict_level(dmax, dist, D.prm.log_scale_factor);       // :315, not clamped
    t.proj_x1 = q.x1; t.proj_y1 = q.y1; t.proj_x2 = q.x2; t.proj_y2 = q.y2; t.scale_level = L; t.view_cos = viewCos;
    float r = ((double)viewCos > 0.998) ? 5.0f : 8.0f;                      // RadiusByViewingCos: float vs double constant
    if (b.th != 1.0f) r *= b.th;                                            // bFactor (:140, :149-150)
    q.r = r * b.scale_factors[clampi(L, 0, b.nlevels - 1)];                   // :153 (level clamped for the lookup only)
    q.minLevel = wrap_add(L, -1); q.maxLevel = L;
    return true;
}

// ---- k_line_query: one lane per line ---------------------------------------------------------------------------------------------------------
template <bool LOCAL>
__global__ __launch_bounds__(256) void k_line_query(LineDev D) {
    const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= min(max(D.nLines[f], 0), D.ncap)) return;
    const size_t ii = (size_t)f * D.ncap + i;
    LineQ q{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0, 0, 0};
    if (LOCAL) {
        msl_line_track t{0.0f, 0.0f, 0.0f, 0.0f, 0, 0.0f};
        const bool in = local_query(D, f, i, q, t);
        if (!in) t = msl_line_track{0.0f, 0.0f, 0.0f, 0.0f, 0, 0.0f};
        q.ok = in;
        D.inView[ii] = in; D.track[ii] = t;
        if (D.inViewOut) D.inViewOut[ii] = in;
        if (D.trackOut) D.trackOut[ii] = t;
    } else {
        q.ok = last_query(D, f, i, q);
    }
    D.q[ii] = q;
}

// ---- k_line_assign: one workgroup per frame -----------------------------------------------------------------------------------------------------
// The reference walks the lines in order; line i scans GetLinesInArea's indices (ascending keyline index k), skips a keyline whose
// mvpMapLines[k] has Observations() > 0, keeps (bestDist, bestLevel, bestIdx) and (bestDist2, bestLevel2) with strict < updates from 256 / -1,
// and writes mvpMapLines[bestIdx] = line i when bestDist <= TH_HIGH and not (bestLevel == bestLevel2 && bestDist > mfNNratio * bestDist2):
// the greedy hand-out of msl_assign.h with lines as queries and keylines as targets.  With the key (dist << 16 | k), the strict-< updates
// leave bestIdx / bestLevel = the smallest key and bestDist2 / bestLevel2 = the second smallest among the keylines line i does not skip
// (distance 256 never passes < 256 and is dropped), so pick(i) is a function of the set of keylines line i skips, as the hand-out requires.
// LDS: keylines 4 KB + descriptors 8 KB + t 1 KB static, pick[ncap] short dynamic (64 KB at mlcap = 32768): 77 KB at the limits.
template <bool LOCAL>
__global__ __launch_bounds__(LINE_NT) void k_line_assign(LineDev D) {
    __shared__ msl_keyline s_kl[MAX_KLCAP];
    __shared__ uint4 s_desc[2 * MAX_KLCAP];
    __shared__ int s_t[MAX_KLCAP];
    __shared__ int s_nm, s_ntm;
    extern __shared__ short s_pick[];               // [ncap]
    const int f = blockIdx.x;
    const int nCur = min(max(D.nCur[f], 0), D.lcap), nL = min(max(D.nLines[f], 0), D.ncap);
    const size_t kb = (size_t)f * D.lcap, lb = (size_t)f * D.ncap;
    for (int k = threadIdx.x; k < nCur; k += LINE_NT) {
        s_kl[k] = D.curKl[kb + k];
        load_desc(D.curDesc + (kb + k) * 32, s_desc[2 * k], s_desc[2 * k + 1]);
    }
    if (threadIdx.x == 0) s_ntm = 0;

    // line i's choice given the current t: GetLinesInArea (src/Frame.cc:384-415) over the keylines it does not skip, then :117-129 / :183-191
    auto pick_of = [&](int i) -> int {
        const LineQ q = D.q[lb + i];
        if (!q.ok) return -1;
        uint4 d0, d1;
        load_desc(D.desc + (lb + i) * 32, d0, d1);
        const double mx = 0.5 * (double)(q.x1 + q.x2), my = 0.5 * (double)(q.y1 + q.y2);   // float sums, then double
        const float slope0 = (q.y1 - q.y2) / (q.x1 - q.x2);
        const float rr = q.r * q.r;
        const double rs = (double)q.r * 0.01;
        const bool bCheckLevels = (q.minLevel > 0) || (q.maxLevel > 0);
        unsigned b1 = K_NONE, b2 = K_NONE;
        for (int k = 0; k < nCur; k++) {
            if (s_t[k] < i) continue;                                       // held by a line with observations
            const msl_keyline kl = s_kl[k];
            const double dx = mx - (double)kl.x, dy = my - (double)kl.y;
            const float distance = (float)(dx * dx + dy * dy);
            if (distance > rr) continue;
            const float slope = slope0 - kl.angle;                          // no fabs: a negative difference, or NaN, passes
            if ((double)slope > rs) continue;
            if (bCheckLevels) {
                if (kl.octave < q.minLevel) continue;
                if (q.maxLevel >= 0 && kl.octave > q.maxLevel) continue;
            }
            const int dist = hamming256(d0, d1, s_desc[2 * k], s_desc[2 * k + 1]);
            if (dist < 256) two_smallest(((unsigned)dist << 16) | (unsigned)k, b1, b2);
        }
        if (b1 == K_NONE) return -1;
        const int bestDist = (int)(b1 >> 16);
        if (bestDist > TH_HIGH) return -1;
        const int bestLevel = s_kl[b1 & 0xFFFFu].octave;
        const int bestLevel2 = b2 == K_NONE ? -1 : s_kl[b2 & 0xFFFFu].octave;
        const int bestDist2 = b2 == K_NONE ? 256 : (int)(b2 >> 16);
        if (bestLevel == bestLevel2 && (float)bestDist > D.prm.nn_ratio * (float)bestDist2) return -1;
        return (int)(b1 & 0xFFFFu);
    };
    // keylines held with observations on entry (cur_line_flags 3, local search only) are skipped by every line
    greedy_assign<LINE_NT>(nL, nCur, s_t, s_pick, &s_nm, pick_of, [&](int i) { return (D.flags[lb + i] & 2) != 0; },
                           [&](int k) { return (LOCAL && (D.curFlags[kb + k] & 3) == 3) ? -1 : T_FREE; });
    if (LOCAL) {
        int ntm = 0;
        for (int i = threadIdx.x; i < nL; i += LINE_NT) ntm += D.inView[lb + i];
        if (ntm) atomicAdd(&s_ntm, ntm);
        __syncthreads();
    }
    for (int k = threadIdx.x; k < D.lcap; k += LINE_NT) {
        const int h = k < nCur ? s_t[k] : -1;
        D.matchOut[kb + k] = h;
        if (k >= nCur) continue;
        if (h >= 0) {
            if (D.lineXyz)
                for (int c = 0; c < 6; c++) D.lineXyz[(kb + k) * 6 + c] = D.xyz[(lb + h) * 6 + c];
            if (D.lineHas) D.lineHas[kb + k] = 1;
        } else if (!LOCAL && D.lineHas) {
            D.lineHas[kb + k] = 0;                                          // the last-frame search starts from all NULL
        }
    }
    if (threadIdx.x == 0) {
        D.nmatches[f] = s_nm;
        if (LOCAL) D.nToMatch[f] = s_ntm;
    }
}

// Whether a _batch form reads device memory the caller may still have enqueued on the legacy stream: its inputs, or the in/out line_xyz /
// line_has (they live in out_mem memory).
bool reads_device(msl_mem mem, const double *line_xyz, const uint8_t *line_has, msl_mem out_mem) {
    return mem == MSL_MEM_DEVICE || ((line_xyz || line_has) && out_mem == MSL_MEM_DEVICE);
}

constexpr const char *WHO_LAST = "msl_match_lines_by_projection", *WHO_LOCAL = "msl_match_local_lines";

// In both checks line_xyz and line_has are optional, each on its own.
int check_lines_last(int n_frames, int lcap, int llcap, const msl_line_match_params *params, const msl_keyline *cur_kl, const uint8_t *cur_ldesc,
                     const int32_t *n_cur_lines, const double *last_line_xyz, const uint8_t *last_ldesc, const uint8_t *last_line_flags,
                     const int32_t *last_line_octave, const int32_t *n_last_lines, const float *Tcw_cur, const float *Tcw_last, msl_mem,
                     int32_t *match_out, int32_t *nmatches, double *, uint8_t *, msl_mem) {
    const char *who = WHO_LAST;
    if (!none_null(who, {MSL_NAMED(params), MSL_NAMED(cur_kl), MSL_NAMED(cur_ldesc), MSL_NAMED(n_cur_lines), MSL_NAMED(last_line_xyz),
                         MSL_NAMED(last_ldesc), MSL_NAMED(last_line_flags), MSL_NAMED(last_line_octave), MSL_NAMED(n_last_lines), MSL_NAMED(Tcw_cur),
                         MSL_NAMED(Tcw_last), MSL_NAMED(match_out), MSL_NAMED(nmatches)})) return MSL_ERR_INVALID;
    if (!at_least_one(who, "n_frames", n_frames) || !in_range(who, "lcap", lcap, 1, MAX_KLCAP) || !in_range(who, "llcap", llcap, 1, MAX_LLCAP) ||
        !frame_ok(who, params->base)) return MSL_ERR_INVALID;
    return MSL_OK;
}

int launch_lines_last(msl_match *h, int n_frames, int lcap, int llcap, const msl_line_match_params *params, const msl_keyline *cur_kl,
                      const uint8_t *cur_ldesc, const int32_t *n_cur_lines, const double *last_line_xyz, const uint8_t *last_ldesc,
                      const uint8_t *last_line_flags, const int32_t *last_line_octave, const int32_t *n_last_lines, const float *Tcw_cur,
                      const float *Tcw_last, msl_mem mem, int32_t *match_out, int32_t *nmatches, double *line_xyz, uint8_t *line_has, msl_mem out_mem) {
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    hipStream_t st = h->stream;
    const size_t F = (size_t)n_frames, l = F * lcap, n = F * llcap;
    Stage S(h, mem, out_mem);
    LineDev D{};
    D.lcap = lcap; D.ncap = llcap; D.prm = *params; D.mb = params->base.bf / params->base.fx;   // src/Frame.cc:150
    D.curKl = S.in(cur_kl, l); D.curDesc = S.in(cur_ldesc, 32 * l); D.nCur = S.in(n_cur_lines, F); D.xyz = S.in(last_line_xyz, 6 * n);
    D.desc = S.in(last_ldesc, 32 * n); D.flags = S.in(last_line_flags, n); D.octave = S.in(last_line_octave, n); D.nLines = S.in(n_last_lines, F);
    D.TcwCur = S.in(Tcw_cur, 12 * F); D.TcwLast = S.in(Tcw_last, 12 * F);
    D.matchOut = S.out(match_out, l); D.nmatches = S.out(nmatches, F);
    D.lineXyz = S.inout(line_xyz, 6 * l); D.lineHas = S.inout(line_has, l);
    MSL_HIP_TRY(S.error());
    MSL_HIP_TRY(grow_all(st, {{h->lineQ, sizeof(LineQ) * n}}));
    D.q = (LineQ *)h->lineQ.p;
    MSL_HIP_TRY(allow_lds(h, LDS_LINE_ASSIGN_LAST, k_line_assign<false>, sizeof(short) * MAX_LLCAP));
    hipLaunchKernelGGL(k_line_query<false>, dim3((unsigned)((llcap + 255) / 256), (unsigned)n_frames), dim3(256), 0, st, D);
    hipLaunchKernelGGL(k_line_assign<false>, dim3((unsigned)n_frames), dim3(LINE_NT), sizeof(short) * llcap, st, D);
    MSL_HIP_TRY(hipGetLastError());
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}

int check_lines_local(int n_frames, int lcap, int mlcap, const msl_line_match_params *params, const msl_keyline *cur_kl, const uint8_t *cur_ldesc,
                      const int32_t *n_cur_lines, const uint8_t *cur_line_flags, const double *ml_xyz, const double *ml_normal, const float *ml_dist,
                      const uint8_t *ml_desc, const uint8_t *ml_flags, const int32_t *n_local_lines, const float *Tcw, msl_mem, int32_t *match_out,
                      int32_t *n_to_match, int32_t *nmatches, uint8_t *, msl_line_track *, double *, uint8_t *, msl_mem) {
    const char *who = WHO_LOCAL;
    if (!none_null(who, {MSL_NAMED(params), MSL_NAMED(cur_kl), MSL_NAMED(cur_ldesc), MSL_NAMED(n_cur_lines), MSL_NAMED(cur_line_flags),
                         MSL_NAMED(ml_xyz), MSL_NAMED(ml_normal), MSL_NAMED(ml_dist), MSL_NAMED(ml_desc), MSL_NAMED(ml_flags), MSL_NAMED(n_local_lines),
                         MSL_NAMED(Tcw), MSL_NAMED(match_out), MSL_NAMED(n_to_match), MSL_NAMED(nmatches)})) return MSL_ERR_INVALID;   // in_view, track: optional
    if (!at_least_one(who, "n_frames", n_frames) || !in_range(who, "lcap", lcap, 1, MAX_KLCAP) || !in_range(who, "mlcap", mlcap, 1, MAX_MCAP) ||
        !frame_ok(who, params->base) || !log_scale_ok(who, params->log_scale_factor)) return MSL_ERR_INVALID;
    return MSL_OK;
}

int launch_lines_local(msl_match *h, int n_frames, int lcap, int mlcap, const msl_line_match_params *params, const msl_keyline *cur_kl,
                       const uint8_t *cur_ldesc, const int32_t *n_cur_lines, const uint8_t *cur_line_flags, const double *ml_xyz, const double *ml_normal,
                       const float *ml_dist, const uint8_t *ml_desc, const uint8_t *ml_flags, const int32_t *n_local_lines, const float *Tcw, msl_mem mem,
                       int32_t *match_out, int32_t *n_to_match, int32_t *nmatches, uint8_t *in_view, msl_line_track *track, double *line_xyz,
                       uint8_t *line_has, msl_mem out_mem) {
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    hipStream_t st = h->stream;
    const size_t F = (size_t)n_frames, l = F * lcap, m = F * mlcap;
    Stage S(h, mem, out_mem);
    LineDev D{};
    D.lcap = lcap; D.ncap = mlcap; D.prm = *params;
    D.curKl = S.in(cur_kl, l); D.curDesc = S.in(cur_ldesc, 32 * l); D.nCur = S.in(n_cur_lines, F); D.curFlags = S.in(cur_line_flags, l);
    D.xyz = S.in(ml_xyz, 6 * m); D.normal = S.in(ml_normal, 3 * m); D.dist = S.in(ml_dist, 2 * m); D.desc = S.in(ml_desc, 32 * m);
    D.flags = S.in(ml_flags, m); D.nLines = S.in(n_local_lines, F); D.TcwCur = S.in(Tcw, 12 * F);
    D.matchOut = S.out(match_out, l); D.nmatches = S.out(nmatches, F); D.nToMatch = S.out(n_to_match, F);
    D.lineXyz = S.inout(line_xyz, 6 * l); D.lineHas = S.inout(line_has, l);
    MSL_HIP_TRY(S.error());
    MSL_HIP_TRY(grow_all(st, {{h->lineQ, sizeof(LineQ) * m}, {h->lineTrk, sizeof(msl_line_track) * m}, {h->lineView, m}}));
    D.q = (LineQ *)h->lineQ.p; D.track = (msl_line_track *)h->lineTrk.p; D.inView = (uint8_t *)h->lineView.p;
    D.inViewOut = S.out_of_scratch(in_view, D.inView, m); D.trackOut = S.out_of_scratch(track, D.track, m);   // the optional in_view / track
    MSL_HIP_TRY(allow_lds(h, LDS_LINE_ASSIGN_LOCAL, k_line_assign<true>, sizeof(short) * MAX_MCAP));
    hipLaunchKernelGGL(k_line_query<true>, dim3((unsigned)((mlcap + 255) / 256), (unsigned)n_frames), dim3(256), 0, st, D);
    hipLaunchKernelGGL(k_line_assign<true>, dim3((unsigned)n_frames), dim3(LINE_NT), sizeof(short) * mlcap, st, D);
    MSL_HIP_TRY(hipGetLastError());
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}

}  // namespace

extern "C" {

int msl_match_lines_by_projection(msl_match *h, int n_frames, int lcap, int llcap, const msl_line_match_params *params, const msl_keyline *cur_kl,
                                  const uint8_t *cur_ldesc, const int32_t *n_cur_lines, const double *last_line_xyz, const uint8_t *last_ldesc,
                                  const uint8_t *last_line_flags, const int32_t *last_line_octave, const int32_t *n_last_lines, const float *Tcw_cur,
                                  const float *Tcw_last, msl_mem mem, int32_t *match_out, int32_t *nmatches, double *line_xyz, uint8_t *line_has,
                                  msl_mem out_mem) noexcept {
    try {
    return handle_form(WHO_LAST, check_lines_last, launch_lines_last, h, n_frames, lcap, llcap, params, cur_kl, cur_ldesc, n_cur_lines, last_line_xyz,
                       last_ldesc, last_line_flags, last_line_octave, n_last_lines, Tcw_cur, Tcw_last, mem, match_out, nmatches, line_xyz, line_has, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_match_lines_by_projection_batch(int device, int n_frames, int lcap, int llcap, const msl_line_match_params *params, const msl_keyline *cur_kl,
                                        const uint8_t *cur_ldesc, const int32_t *n_cur_lines, const double *last_line_xyz, const uint8_t *last_ldesc,
                                        const uint8_t *last_line_flags, const int32_t *last_line_octave, const int32_t *n_last_lines,
                                        const float *Tcw_cur, const float *Tcw_last, msl_mem mem, int32_t *match_out, int32_t *nmatches,
                                        double *line_xyz, uint8_t *line_has, msl_mem out_mem) noexcept {
    try {
    return batch_form(check_lines_last, launch_lines_last, device, reads_device(mem, line_xyz, line_has, out_mem), n_frames, lcap, llcap, params, cur_kl,
                      cur_ldesc, n_cur_lines, last_line_xyz, last_ldesc, last_line_flags, last_line_octave, n_last_lines, Tcw_cur, Tcw_last, mem, match_out,
                      nmatches, line_xyz, line_has, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_match_local_lines(msl_match *h, int n_frames, int lcap, int mlcap, const msl_line_match_params *params, const msl_keyline *cur_kl,
                          const uint8_t *cur_ldesc, const int32_t *n_cur_lines, const uint8_t *cur_line_flags, const double *ml_xyz,
                          const double *ml_normal, const float *ml_dist, const uint8_t *ml_desc, const uint8_t *ml_flags, const int32_t *n_local_lines,
                          const float *Tcw, msl_mem mem, int32_t *match_out, int32_t *n_to_match, int32_t *nmatches, uint8_t *in_view,
                          msl_line_track *track, double *line_xyz, uint8_t *line_has, msl_mem out_mem) noexcept {
    try {
    return handle_form(WHO_LOCAL, check_lines_local, launch_lines_local, h, n_frames, lcap, mlcap, params, cur_kl, cur_ldesc, n_cur_lines, cur_line_flags,
                       ml_xyz, ml_normal, ml_dist, ml_desc, ml_flags, n_local_lines, Tcw, mem, match_out, n_to_match, nmatches, in_view, track, line_xyz,
                       line_has, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_match_local_lines_batch(int device, int n_frames, int lcap, int mlcap, const msl_line_match_params *params, const msl_keyline *cur_kl,
                                const uint8_t *cur_ldesc, const int32_t *n_cur_lines, const uint8_t *cur_line_flags, const double *ml_xyz,
                                const double *ml_normal, const float *ml_dist, const uint8_t *ml_desc, const uint8_t *ml_flags,
                                const int32_t *n_local_lines, const float *Tcw, msl_mem mem, int32_t *match_out, int32_t *n_to_match, int32_t *nmatches,
                                uint8_t *in_view, msl_line_track *track, double *line_xyz, uint8_t *line_has, msl_mem out_mem) noexcept {
    try {
    return batch_form(check_lines_local, launch_lines_local, device, reads_device(mem, line_xyz, line_has, out_mem), n_frames, lcap, mlcap, params, cur_kl,
                      cur_ldesc, n_cur_lines, cur_line_flags, ml_xyz, ml_normal, ml_dist, ml_desc, ml_flags, n_local_lines, Tcw, mem, match_out, n_to_match,
                      nmatches, in_view, track, line_xyz, line_has, out_mem);
    } MSL_ABI_CATCH_INT
}

}  // extern "C"

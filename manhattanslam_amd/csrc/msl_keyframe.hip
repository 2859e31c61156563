// msl_keyframe.hip -- the hand-over from tracking to local mapping for gfx950: the tail of Tracking::TrackLocalMap (reference
// src/Tracking.cc:1365-1430), mbNewPlane (:429-436), "Clean VO matches" (:450-465) and Tracking::NeedNewKeyFrame (:1433-1508) with
// KeyFrame::TrackedMapPoints (src/KeyFrame.cc:199-218) as msl_keyframe_decision[_batch]; the point half of StereoInitialization (:560-572),
// UpdateLastFrame (:1062-1104) and CreateNewKeyFrame (:1524-1569) with Frame::UnprojectStereo (src/Frame.cc:515-526) and the two MapPoint
// constructors (src/MapPoint.cc:36-71) as msl_points_3d[_batch].
//
// Kernels (one workgroup per frame):
//   k_points3d   1024 threads.  The members (slots with depth > 0) as (float bits << 32 | index) keys in LDS -- positive floats order as their
//                bits, the index breaks ties as std::sort of pair<float, int> does; MSL_POINT3D_ALL keys are the index alone -- sorted by
//                bitonic_sort over the power of two at or above the frame's n_kps.  The length of the walk is the closed form
//                min(M, max(#members with !(z > th_depth), min_points) + 1): the members are ascending, so the first position p with
//                z_p > th_depth && p + 1 > min_points is max(#near, min_points).  The walked members, 1024 at a time: fresh or held, a block
//                scan of the fresh ones gives the creation rank j, the thread builds the point of its member and writes its slot with
//                vector stores.  A byte per slot in LDS says which slots got a point; the others are written once, afterwards.
//                LDS: 8 bytes per key and 1 byte per slot, 72 KiB at cap = 8192: two workgroups fit the CU's 160 KiB, and two workgroups of
//                16 waves are the CU's 32 waves, so LDS does not lower the occupancy the workgroup size already sets.
//   k_kf_decide  256 threads.  Integers in LDS counters (atomicAdd: the sums do not depend on the order) and the float comparisons of
//                NeedNewKeyFrame in the reference's types, by thread 0.
// Pins (tests/keyframe_model.py is the sequential model; contraction off): msl.h's list.
#include "msl_match_handle.h"
#include "msl_index_check.h"
#include "msl_match_math.h"
#include "msl_plane_tables.h"

namespace {

using namespace msl;

constexpr int P3_NT = 1024, KD_NT = 256;
const char *const WHO_P3 = "msl_points_3d", *const WHO_KD = "msl_keyframe_decision";

// ==== msl_points_3d ==========================================================================================================================
struct Pts3dDev {
    int cap, nPts, mode, P;
    msl_point3d_params prm;
    float invfx, invfy;
    const msl_keypoint *kps; const float *depth; const uint8_t *desc; const int32_t *nKps, *held, *nobs; const float *Tcw;
    const int32_t *enable, *firstId;
    uint8_t *ptNew, *cleared; float *xyz, *normal, *dist; uint8_t *newDesc; int32_t *heldOut, *order, *nNew, *nWalked;
};

// The point of slot g = f * cap + i: Frame::UnprojectStereo, then what its constructor (and, in the KeyFrame form, AddObservation,
// ComputeDistinctiveDescriptors and UpdateNormalAndDepth with this one observation) leaves in mWorldPos, mNormalVector, mfMin/MaxDistance.
__device__ __forceinline__ void build_point(const Pts3dDev &D, size_t f, size_t g, float X[3], float normal[3], float dist[2]) {
    const msl_keypoint kp = D.kps[g];
    const float z = D.depth[g];
    const float x = (kp.x - D.prm.cx) * z * D.invfx, y = (kp.y - D.prm.cy) * z * D.invfy;
    const float *T = D.Tcw + f * 12;
    float Ow[3], v[3];
    camera_centre(T, Ow);                                                      // mOw = -mRcw.t() * mtcw
    const float Xc[3] = {x, y, z};
    gemm3(T, true, 1.0, Xc, Ow, X);                                            // mRwc * x3Dc + mOw
#pragma unroll
    for (int a = 0; a < 3; a++) v[a] = X[a] - Ow[a];
    const double nrm = norm3_dacc(v), inv = 1.0 / nrm;
    const bool levelOk = kp.octave >= 0 && kp.octave < D.prm.nlevels;
    const bool frameForm = D.mode == MSL_POINT3D_FRAME;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float t = (float)((double)v[a] * inv);                           // normali / cv::norm(normali)
        float acc = 0.0f;
        acc = acc + t;                                                         // normal = normal + ...: a -0 becomes +0
        const float kf = (float)((double)acc * (1.0 / 1.0));                   // normal / n with n = 1
        normal[a] = frameForm ? t : (levelOk ? kf : 0.0f);                     // UpdateNormalAndDepth writes nothing for a bad octave (pin)
    }
    dist[0] = dist[1] = 0.0f;
    if (levelOk) {
        dist[1] = (float)nrm * D.prm.scale_factors[kp.octave];
        dist[0] = dist[1] / D.prm.scale_factors[D.prm.nlevels - 1];
    }
}

__global__ __launch_bounds__(P3_NT) void k_points3d(Pts3dDev D) {
    extern __shared__ unsigned long long s_key[];                              // [P] keys, then [cap] bytes: 1 where the slot got a point
    __shared__ int s_members, s_near;
    __shared__ unsigned s_wave[17];
    const size_t f = blockIdx.x, fb = f * D.cap;
    const int tid = threadIdx.x, cap = D.cap;
    uint8_t *s_made = reinterpret_cast<uint8_t *>(s_key + D.P);
    const bool all = D.mode == MSL_POINT3D_ALL;
    const int n = clampi(D.nKps[f], 0, cap);
    const int nm = (!D.enable || D.enable[f] != 0) ? n : 0;                     // a frame that is not enabled has no members
    const int Pf = pow2_at_least(nm > 2 ? nm : 2);
    if (tid == 0) { s_members = 0; s_near = 0; }
    for (int i = tid; i < cap; i += P3_NT) s_made[i] = 0;
    __syncthreads();
    int members = 0, near = 0;
    for (int i = tid; i < Pf; i += P3_NT) {
        unsigned long long key = ~0ull;
        if (i < nm) {
            const float z = D.depth[fb + i];
            if (z > 0) {                                                       // a NaN is no member, +inf is one
                key = ((unsigned long long)(all ? 0u : __float_as_uint(z)) << 32) | (unsigned)i;
                members++;
                near += z > D.prm.th_depth ? 0 : 1;
            }
        }
        s_key[i] = key;
    }
    members = wave_sum(members); near = wave_sum(near);
    if (lane_id() == 0 && members) { atomicAdd(&s_members, members); atomicAdd(&s_near, near); }
    bitonic_sort(s_key, Pf);                                                   // barriers before the first read and after the last write
    const int M = s_members;
    int L = M;                                                                 // the members the walk handles: the reference's nPoints
    if (!all) {
        const int cut = s_near > D.prm.min_points ? s_near : D.prm.min_points;
        L = cut < M ? cut + 1 : M;
    }
    unsigned made = 0;
    for (int base = 0; base < L; base += P3_NT) {
        const int p = base + tid;
        bool fresh = false, clr = false;
        int i = 0;
        if (p < L) {
            i = (int)(s_key[p] & 0xFFFFFFFFull);
            fresh = true;
            if (!all) {
                const int id = D.held[fb + i];
                const bool held = id >= 0 && id < D.nPts;
                clr = held && D.nobs[id] < 1;
                fresh = !held || clr;
            }
        }
        unsigned total;
        const unsigned j = made + block_excl_scan(fresh ? 1u : 0u, s_wave, &total);
        if (fresh) {
            const size_t g = fb + i;
            float X[3], normal[3], dist[2];
            build_point(D, f, g, X, normal, dist);
            uint4 d0, d1;
            load_desc(D.desc + g * 32, d0, d1);
            D.ptNew[g] = 1; D.cleared[g] = clr ? 1 : 0;
#pragma unroll
            for (int a = 0; a < 3; a++) { D.xyz[3 * g + a] = X[a]; D.normal[3 * g + a] = normal[a]; }
            D.dist[2 * g] = dist[0]; D.dist[2 * g + 1] = dist[1];
            reinterpret_cast<uint4 *>(D.newDesc + g * 32)[0] = d0; reinterpret_cast<uint4 *>(D.newDesc + g * 32)[1] = d1;
            D.heldOut[g] = D.firstId ? D.firstId[f] + (int)j : -1;
            D.order[fb + j] = i;
            s_made[i] = 1;
        }
        made += total;
    }
    __syncthreads();
    const uint4 zero = make_uint4(0, 0, 0, 0);
    for (int i = tid; i < cap; i += P3_NT) {
        const size_t g = fb + i;
        if (!s_made[i]) {
            D.ptNew[g] = 0; D.cleared[g] = 0;
#pragma unroll
            for (int a = 0; a < 3; a++) { D.xyz[3 * g + a] = 0.0f; D.normal[3 * g + a] = 0.0f; }
            D.dist[2 * g] = 0.0f; D.dist[2 * g + 1] = 0.0f;
            reinterpret_cast<uint4 *>(D.newDesc + g * 32)[0] = zero; reinterpret_cast<uint4 *>(D.newDesc + g * 32)[1] = zero;
            D.heldOut[g] = (!all && i < n) ? D.held[g] : -1;
        }
        if ((unsigned)i >= made) D.order[g] = -1;
    }
    if (tid == 0) { D.nNew[f] = (int)made; D.nWalked[f] = L; }
}

int check_points3d(int n_frames, int cap, int n_pts, int mode, const msl_point3d_params *params, const msl_keypoint *kps_un, const float *depth,
                   const uint8_t *desc, const int32_t *n_kps, const int32_t *cur_held, const int32_t *pt_nobs, const float *Tcw,
                   const int32_t *, const int32_t *, msl_mem mem, uint8_t *pt_new, uint8_t *cleared, float *new_xyz, float *new_normal,
                   float *new_dist, uint8_t *new_desc, int32_t *held_out, int32_t *new_order, int32_t *n_new, int32_t *n_walked, msl_mem) {
    const char *who = WHO_P3;
    if (!none_null(who, {MSL_NAMED(params), MSL_NAMED(kps_un), MSL_NAMED(depth), MSL_NAMED(desc), MSL_NAMED(n_kps), MSL_NAMED(Tcw), MSL_NAMED(pt_new),
                         MSL_NAMED(cleared), MSL_NAMED(new_xyz), MSL_NAMED(new_normal), MSL_NAMED(new_dist), MSL_NAMED(new_desc),
                         MSL_NAMED(held_out), MSL_NAMED(new_order), MSL_NAMED(n_new), MSL_NAMED(n_walked)})) return MSL_ERR_INVALID;
    if (n_frames < 1) { set_error("%s: n_frames %d below 1", who, n_frames); return MSL_ERR_INVALID; }
    if (!in_range(who, "cap", cap, 1, MAX_CAP) || !in_range(who, "n_pts", n_pts, 0, MAX_PTS)) return MSL_ERR_INVALID;
    if (mode < MSL_POINT3D_ALL || mode > MSL_POINT3D_FRAME) { set_error("%s: mode %d is not an MSL_POINT3D_* value", who, mode); return MSL_ERR_INVALID; }
    if (!levels_ok(who, params->nlevels)) return MSL_ERR_INVALID;
    if (params->min_points < 0) { set_error("%s: min_points %d below 0", who, params->min_points); return MSL_ERR_INVALID; }
    const bool all = mode == MSL_POINT3D_ALL;
    if (!all && !none_null(who, {MSL_NAMED(cur_held)})) return MSL_ERR_INVALID;
    if (!all && n_pts > 0 && !none_null(who, {MSL_NAMED(pt_nobs)})) return MSL_ERR_INVALID;
    char why[256];
    if (mem == MSL_MEM_HOST) {
        if (!all && !check::held_ok("cur_held", "n_kps", n_frames, cap, n_pts, cur_held, n_kps, why, sizeof(why))) return refuse(who, why);
        for (int f = 0; all && f < n_frames; f++)
            if (n_kps[f] < 0 || n_kps[f] > cap) { set_error("%s: n_kps[%d] is %d outside 0 .. %d", who, f, (int)n_kps[f], cap); return MSL_ERR_INVALID; }
    }
    return MSL_OK;
}

int launch_points3d(msl_match *h, int n_frames, int cap, int n_pts, int mode, const msl_point3d_params *prm, const msl_keypoint *kps_un,
                    const float *depth, const uint8_t *desc, const int32_t *n_kps, const int32_t *cur_held, const int32_t *pt_nobs, const float *Tcw,
                    const int32_t *enable, const int32_t *first_id, msl_mem mem, uint8_t *pt_new, uint8_t *cleared, float *new_xyz,
                    float *new_normal, float *new_dist, uint8_t *new_desc, int32_t *held_out, int32_t *new_order, int32_t *n_new,
                    int32_t *n_walked, msl_mem out_mem) {
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    const size_t F = (size_t)n_frames, n = F * cap;
    const bool all = mode == MSL_POINT3D_ALL;
    Pts3dDev D{};
    D.cap = cap; D.nPts = n_pts; D.mode = mode; D.P = pow2_at_least(cap > 2 ? cap : 2);
    D.prm = *prm; D.invfx = 1.0f / prm->fx; D.invfy = 1.0f / prm->fy;
    Stage S(h, mem, out_mem);
    D.kps = S.in(kps_un, n); D.depth = S.in(depth, n); D.desc = S.in(desc, 32 * n); D.nKps = S.in(n_kps, F);
    D.held = S.in(all ? nullptr : cur_held, n); D.nobs = S.in(all || !n_pts ? nullptr : pt_nobs, (size_t)n_pts); D.Tcw = S.in(Tcw, 12 * F);
    D.enable = S.in(enable, F); D.firstId = S.in(first_id, F);
    D.ptNew = S.out(pt_new, n); D.cleared = S.out(cleared, n); D.xyz = S.out(new_xyz, 3 * n); D.normal = S.out(new_normal, 3 * n);
    D.dist = S.out(new_dist, 2 * n); D.newDesc = S.out(new_desc, 32 * n); D.heldOut = S.out(held_out, n); D.order = S.out(new_order, n);
    D.nNew = S.out(n_new, F); D.nWalked = S.out(n_walked, F);
    MSL_HIP_TRY(S.error());
    MSL_HIP_TRY(allow_lds(h, LDS_POINTS3D, k_points3d, 9 * (size_t)MAX_CAP));
    hipLaunchKernelGGL(k_points3d, dim3((unsigned)n_frames), dim3(P3_NT), 8 * (size_t)D.P + (size_t)cap, h->stream, D);
    MSL_HIP_TRY(hipGetLastError());
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}

// ==== msl_keyframe_decision ==================================================================================================================
struct DecideDev {
    int cap, lcap, pcap, nTab, nPts, nLines;
    msl_keyframe_params prm;
    const msl_keyframe_frame *frames;
    const float *depth; const int32_t *nCur, *held; const uint8_t *outlier;
    const int32_t *lheld; const uint8_t *lineOutlier; const int32_t *nCurLines, *nPlanes;
    const int32_t *ptNobs; const uint8_t *ptFlags; const int32_t *lnNobs, *tabHeld, *tabN;
    int32_t *planeMatch; uint8_t *planeOutlier;
    uint8_t *foundPt, *foundLine; int32_t *nInliers; uint8_t *trackOk, *newPlane;
    int32_t *heldOut; uint8_t *outlierOut; int32_t *lheldOut; uint8_t *lineOutlierOut;
    int32_t *counts; uint8_t *cond; int32_t *needKf;
};

// IncreaseFound() and the mnMatchesInliers share of one kind of element (points or lines), n slots: returns this thread's inliers
__device__ __forceinline__ int tally(bool ran, bool onlyTracking, int n, int cap, int nIds, const int32_t *held, const uint8_t *outlier,
                                     const int32_t *nobs, uint8_t *found) {
    int inl = 0;
    for (int i = threadIdx.x; i < cap; i += KD_NT) {
        bool fnd = false;
        if (ran && i < n) {
            const int id = held[i];
            if (id >= 0 && id < nIds && !outlier[i]) {
                fnd = true;
                inl += (onlyTracking || nobs[id] > 0) ? 1 : 0;
            }
        }
        found[i] = fnd ? 1 : 0;
    }
    return inl;
}

// "Clean VO matches" of one kind of element: the cleaned slot and outlier byte (copies where the frame is not cleaned; -1 / 0 beyond n)
__device__ __forceinline__ void clean(bool ok, int n, int cap, int nIds, const int32_t *held, const uint8_t *outlier, const int32_t *nobs,
                                      int32_t *heldOut, uint8_t *outlierOut) {
    for (int i = threadIdx.x; i < cap; i += KD_NT) {
        int id = -1; uint8_t o = 0;
        if (i < n) {
            id = held[i]; o = outlier[i];
            if (ok && id >= 0 && id < nIds && nobs[id] < 1) { id = -1; o = 0; }
        }
        heldOut[i] = id; outlierOut[i] = o;
    }
}

__global__ __launch_bounds__(KD_NT) void k_kf_decide(DecideDev D) {
    __shared__ int s_inl, s_newPlane, s_ref, s_total, s_map, s_ok;
    const size_t f = blockIdx.x;
    const int tid = threadIdx.x;
    const msl_keyframe_frame R = D.frames[f];
    const bool ran = R.flags & MSL_KF_TRACKED_LOCAL_MAP, onlyTracking = D.prm.only_tracking != 0;
    const int n = clampi(D.nCur[f], 0, D.cap), nl = clampi(D.nCurLines[f], 0, D.lcap), np = clampi(D.nPlanes[f], 0, D.pcap);
    const size_t pb = f * D.cap, lb = f * D.lcap, qb = f * D.pcap * 3;
    if (tid == 0) { s_inl = 0; s_newPlane = (!ran && (R.flags & MSL_KF_NEW_PLANE)) ? 1 : 0; s_ref = 0; s_total = 0; s_map = 0; }
    __syncthreads();
    // ---- step 1: the tail of TrackLocalMap ----
    int inl = tally(ran, onlyTracking, n, D.cap, D.nPts, D.held + pb, D.outlier + pb, D.ptNobs, D.foundPt + pb);
    inl += tally(ran, onlyTracking, nl, D.lcap, D.nLines, D.lheld + lb, D.lineOutlier + lb, D.lnNobs, D.foundLine + lb);
    // ---- the planes: step 1's clean-up, then step 2 (mbNewPlane) on what it left; plane k is thread k's ----
    for (int k = tid; k < np; k += KD_NT) {
        int32_t *m = D.planeMatch + qb + 3 * k; uint8_t *o = D.planeOutlier + qb + 3 * k;
        int m0 = m[0];
        if (ran) {
            if (m0 >= 0) {
                if (o[0]) { m0 = -1; m[0] = -1; }                              // the outlier byte stays
                else inl++;
            }
            for (int s = 1; s < 3; s++)
                if (m[s] >= 0 && o[s]) { m[s] = -1; o[s] = 0; }
        }
        if (m0 < 0 && !o[0]) atomicOr(&s_newPlane, 1);
    }
    inl = wave_sum(inl);
    if (lane_id() == 0 && inl) atomicAdd(&s_inl, inl);
    __syncthreads();
    if (tid == 0) {
        int ok = (R.flags & MSL_KF_TRACK_OK) ? 1 : 0;
        if (ran) {
            // unsigned int + int, compared with the unsigned long mnId: the sum wraps at 2^32
            const unsigned lim = (unsigned)R.last_reloc_frame_id + (unsigned)D.prm.max_frames;
            ok = !((unsigned)R.frame_id < lim && s_inl < 20) && !(s_inl < 7);
        } else s_inl = R.n_inliers_in;
        s_ok = ok;
    }
    __syncthreads();
    const bool ok = s_ok != 0;
    const int inliers = s_inl;
    // ---- step 3: Clean VO matches ----
    clean(ok, n, D.cap, D.nPts, D.held + pb, D.outlier + pb, D.ptNobs, D.heldOut + pb, D.outlierOut + pb);
    clean(ok, nl, D.lcap, D.nLines, D.lheld + lb, D.lineOutlier + lb, D.lnNobs, D.lheldOut + lb, D.lineOutlierOut + lb);
    // ---- step 4: NeedNewKeyFrame ----
    const unsigned id = (unsigned)R.frame_id, maxF = (unsigned)D.prm.max_frames;
    const bool early = !ok || onlyTracking || R.local_mapping_stopped != 0 ||
                       (id < (unsigned)R.last_reloc_frame_id + maxF && R.n_kfs > D.prm.max_frames);
    if (!early) {                                                              // uniform
        const int minObs = R.n_kfs <= 2 ? 2 : 3;
        int ref = 0, total = 0, map = 0;
        if (R.ref_kf >= 0 && R.ref_kf < D.nTab) {                              // KeyFrame::TrackedMapPoints(nMinObs)
            const int nr = clampi(D.tabN[R.ref_kf], 0, D.cap);
            for (int i = tid; i < nr; i += KD_NT) {
                const int p = D.tabHeld[(size_t)R.ref_kf * D.cap + i];
                ref += (p >= 0 && p < D.nPts && (D.ptFlags[p] & 1) && D.ptNobs[p] >= minObs) ? 1 : 0;
            }
        }
        for (int i = tid; i < n; i += KD_NT) {                                 // the cleaned slot, formed again from the inputs: no global read-back
            const float z = D.depth[pb + i];
            if (z > 0 && z < D.prm.th_depth) {
                total++;
                int p = D.held[pb + i];
                bool out = D.outlier[pb + i] != 0;
                const bool held = p >= 0 && p < D.nPts;
                if (held && D.ptNobs[p] < 1) { p = -1; out = false; }
                map += (held && p >= 0 && !out) ? 1 : 0;
            }
        }
        ref = wave_sum(ref); total = wave_sum(total); map = wave_sum(map);
        if (lane_id() == 0) { if (ref) atomicAdd(&s_ref, ref); if (total) atomicAdd(&s_total, total); if (map) atomicAdd(&s_map, map); }
    }
    __syncthreads();
    if (tid == 0) {
        int cnt[4] = {0, 0, 0, 0}, cond = 0, need = 0;
        if (!early) {
            const int nRef = s_ref, nTotal = s_total, nMap = s_map;
            cnt[0] = nRef; cnt[1] = nTotal; cnt[2] = nMap; cnt[3] = nTotal - nMap;
            const double den = (double)nTotal > 1.0 ? (double)nTotal : 1.0;    // fmax(1.0f, int): the double overload
            const float ratioMap = (float)((double)(float)nMap / den);
            const float thRefRatio = R.n_kfs < 2 ? 0.4f : 0.75f, thMapRatio = inliers > 300 ? 0.20f : 0.35f;
            const bool c1a = id >= (unsigned)R.last_keyframe_id + maxF;
            const bool c1b = id >= (unsigned)R.last_keyframe_id + (unsigned)D.prm.min_frames && R.local_mapping_idle != 0;
            const bool c1c = (double)inliers < (double)nRef * 0.25 || ratioMap < 0.3f;
            const bool c2 = ((float)inliers < (float)nRef * thRefRatio || ratioMap < thMapRatio) && inliers > 15;
            cond = (c1a ? MSL_KF_C1A : 0) | (c1b ? MSL_KF_C1B : 0) | (c1c ? MSL_KF_C1C : 0) | (c2 ? MSL_KF_C2 : 0);
            if (((c1a || c1b || c1c) && c2) || s_newPlane) need = R.local_mapping_idle != 0 || R.keyframes_in_queue < 3;
        }
        D.nInliers[f] = inliers; D.trackOk[f] = ok ? 1 : 0; D.newPlane[f] = s_newPlane ? 1 : 0;
        for (int c = 0; c < 4; c++) D.counts[4 * f + c] = cnt[c];
        D.cond[f] = (uint8_t)cond; D.needKf[f] = need;
    }
}

int check_decision(int n_frames, int cap, int lcap, int pcap, int n_tab, int n_pts, int n_lines, const msl_keyframe_params *params,
                   const msl_keyframe_frame *frames, const float *depth, const int32_t *n_cur, const int32_t *cur_held, const uint8_t *outlier,
                   const int32_t *cur_lheld, const uint8_t *line_outlier, const int32_t *n_cur_lines, const int32_t *n_planes,
                   const int32_t *pt_nobs, const uint8_t *pt_flags, const int32_t *ln_nobs, const int32_t *held_id, const int32_t *n_kps, msl_mem mem,
                   int32_t *plane_match, uint8_t *plane_outlier, uint8_t *found_pt, uint8_t *found_line, int32_t *n_inliers, uint8_t *track_ok,
                   uint8_t *new_plane, int32_t *held_out, uint8_t *outlier_out, int32_t *lheld_out, uint8_t *line_outlier_out, int32_t *counts,
                   uint8_t *cond, int32_t *need_kf, msl_mem) {
    const char *who = WHO_KD;
    if (!none_null(who, {MSL_NAMED(params), MSL_NAMED(frames), MSL_NAMED(depth), MSL_NAMED(n_cur), MSL_NAMED(cur_held), MSL_NAMED(outlier),
                         MSL_NAMED(cur_lheld), MSL_NAMED(line_outlier), MSL_NAMED(n_cur_lines), MSL_NAMED(n_planes), MSL_NAMED(pt_nobs),
                         MSL_NAMED(pt_flags), MSL_NAMED(ln_nobs), MSL_NAMED(held_id), MSL_NAMED(n_kps), MSL_NAMED(plane_match),
                         MSL_NAMED(plane_outlier), MSL_NAMED(found_pt), MSL_NAMED(found_line), MSL_NAMED(n_inliers), MSL_NAMED(track_ok),
                         MSL_NAMED(new_plane), MSL_NAMED(held_out), MSL_NAMED(outlier_out), MSL_NAMED(lheld_out), MSL_NAMED(line_outlier_out),
                         MSL_NAMED(counts), MSL_NAMED(cond), MSL_NAMED(need_kf)})) return MSL_ERR_INVALID;
    if (n_frames < 1) { set_error("%s: n_frames %d below 1", who, n_frames); return MSL_ERR_INVALID; }
    if (!in_range(who, "lcap", lcap, 1, MAX_KLCAP) || !in_range(who, "pcap", pcap, 1, MAX_PCAP) || !table_limits(who, n_tab, cap, n_pts) ||
        !in_range(who, "n_lines", n_lines, 1, MAX_LINES)) return MSL_ERR_INVALID;
    char why[256];
    if (mem == MSL_MEM_HOST) {
        if (!check::held_ok("cur_held", "n_cur", n_frames, cap, n_pts, cur_held, n_cur, why, sizeof(why)) ||
            !check::held_ok("cur_lheld", "n_cur_lines", n_frames, lcap, n_lines, cur_lheld, n_cur_lines, why, sizeof(why)) ||
            !check::held_ok("held_id", "n_kps", n_tab, cap, n_pts, held_id, n_kps, why, sizeof(why))) return refuse(who, why);
        for (int f = 0; f < n_frames; f++) {
            if (n_planes[f] < 0 || n_planes[f] > pcap) { set_error("%s: n_planes[%d] is %d outside 0 .. %d", who, f, (int)n_planes[f], pcap); return MSL_ERR_INVALID; }
            if (frames[f].ref_kf < -1 || frames[f].ref_kf >= n_tab) { set_error("%s: frames[%d].ref_kf is keyframe %d of %d", who, f, (int)frames[f].ref_kf, n_tab); return MSL_ERR_INVALID; }
        }
    }
    return MSL_OK;
}

int launch_decision(msl_match *h, int n_frames, int cap, int lcap, int pcap, int n_tab, int n_pts, int n_lines, const msl_keyframe_params *prm,
                    const msl_keyframe_frame *frames, const float *depth, const int32_t *n_cur, const int32_t *cur_held, const uint8_t *outlier,
                    const int32_t *cur_lheld, const uint8_t *line_outlier, const int32_t *n_cur_lines, const int32_t *n_planes,
                    const int32_t *pt_nobs, const uint8_t *pt_flags, const int32_t *ln_nobs, const int32_t *held_id, const int32_t *n_kps,
                    msl_mem mem, int32_t *plane_match, uint8_t *plane_outlier, uint8_t *found_pt, uint8_t *found_line, int32_t *n_inliers,
                    uint8_t *track_ok, uint8_t *new_plane, int32_t *held_out, uint8_t *outlier_out, int32_t *lheld_out, uint8_t *line_outlier_out,
                    int32_t *counts, uint8_t *cond, int32_t *need_kf, msl_mem out_mem) {
    int rc = bind_device(h->device);
    if (rc != MSL_OK) return rc;
    const size_t F = (size_t)n_frames, n = F * cap, nl = F * lcap, q = F * pcap * 3, T = (size_t)n_tab;
    DecideDev D{};
    D.cap = cap; D.lcap = lcap; D.pcap = pcap; D.nTab = n_tab; D.nPts = n_pts; D.nLines = n_lines; D.prm = *prm;
    Stage S(h, mem, out_mem);
    D.frames = S.in(frames, F); D.depth = S.in(depth, n); D.nCur = S.in(n_cur, F); D.held = S.in(cur_held, n); D.outlier = S.in(outlier, n);
    D.lheld = S.in(cur_lheld, nl); D.lineOutlier = S.in(line_outlier, nl); D.nCurLines = S.in(n_cur_lines, F); D.nPlanes = S.in(n_planes, F);
    D.ptNobs = S.in(pt_nobs, (size_t)n_pts); D.ptFlags = S.in(pt_flags, (size_t)n_pts); D.lnNobs = S.in(ln_nobs, (size_t)n_lines);
    D.tabHeld = S.in(held_id, T * cap); D.tabN = S.in(n_kps, T);
    D.planeMatch = S.inout(plane_match, q); D.planeOutlier = S.inout(plane_outlier, q);
    D.foundPt = S.out(found_pt, n); D.foundLine = S.out(found_line, nl); D.nInliers = S.out(n_inliers, F); D.trackOk = S.out(track_ok, F);
    D.newPlane = S.out(new_plane, F); D.heldOut = S.out(held_out, n); D.outlierOut = S.out(outlier_out, n); D.lheldOut = S.out(lheld_out, nl);
    D.lineOutlierOut = S.out(line_outlier_out, nl); D.counts = S.out(counts, 4 * F); D.cond = S.out(cond, F); D.needKf = S.out(need_kf, F);
    MSL_HIP_TRY(S.error());
    hipLaunchKernelGGL(k_kf_decide, dim3((unsigned)n_frames), dim3(KD_NT), 0, h->stream, D);
    MSL_HIP_TRY(hipGetLastError());
    MSL_HIP_TRY(S.finish());
    return MSL_OK;
}

}  // namespace

extern "C" {

int msl_points_3d(msl_match *h, int n_frames, int cap, int n_pts, int mode, const msl_point3d_params *params, const msl_keypoint *kps_un,
                  const float *depth, const uint8_t *desc, const int32_t *n_kps, const int32_t *cur_held, const int32_t *pt_nobs, const float *Tcw,
                  const int32_t *enable, const int32_t *first_id, msl_mem mem, uint8_t *pt_new, uint8_t *cleared, float *new_xyz,
                  float *new_normal, float *new_dist, uint8_t *new_desc, int32_t *held_out, int32_t *new_order, int32_t *n_new, int32_t *n_walked,
                  msl_mem out_mem) noexcept {
    try {
    return handle_form(WHO_P3, check_points3d, launch_points3d, h, n_frames, cap, n_pts, mode, params, kps_un, depth, desc, n_kps, cur_held, pt_nobs,
                       Tcw, enable, first_id, mem, pt_new, cleared, new_xyz, new_normal, new_dist, new_desc, held_out, new_order, n_new, n_walked,
                       out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_points_3d_batch(int device, int n_frames, int cap, int n_pts, int mode, const msl_point3d_params *params, const msl_keypoint *kps_un,
                        const float *depth, const uint8_t *desc, const int32_t *n_kps, const int32_t *cur_held, const int32_t *pt_nobs,
                        const float *Tcw, const int32_t *enable, const int32_t *first_id, msl_mem mem, uint8_t *pt_new, uint8_t *cleared,
                        float *new_xyz, float *new_normal, float *new_dist, uint8_t *new_desc, int32_t *held_out, int32_t *new_order,
                        int32_t *n_new, int32_t *n_walked, msl_mem out_mem) noexcept {
    try {
    return batch_form(check_points3d, launch_points3d, device, mem == MSL_MEM_DEVICE || out_mem == MSL_MEM_DEVICE, n_frames, cap, n_pts, mode, params,
                      kps_un, depth, desc, n_kps, cur_held, pt_nobs, Tcw, enable, first_id, mem, pt_new, cleared, new_xyz, new_normal, new_dist,
                      new_desc, held_out, new_order, n_new, n_walked, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_keyframe_decision(msl_match *h, int n_frames, int cap, int lcap, int pcap, int n_tab, int n_pts, int n_lines,
                          const msl_keyframe_params *params, const msl_keyframe_frame *frames, const float *depth, const int32_t *n_cur,
                          const int32_t *cur_held, const uint8_t *outlier, const int32_t *cur_lheld, const uint8_t *line_outlier,
                          const int32_t *n_cur_lines, const int32_t *n_planes, const int32_t *pt_nobs, const uint8_t *pt_flags,
                          const int32_t *ln_nobs, const int32_t *held_id, const int32_t *n_kps, msl_mem mem, int32_t *plane_match,
                          uint8_t *plane_outlier, uint8_t *found_pt, uint8_t *found_line, int32_t *n_inliers, uint8_t *track_ok, uint8_t *new_plane,
                          int32_t *held_out, uint8_t *outlier_out, int32_t *lheld_out, uint8_t *line_outlier_out, int32_t *counts, uint8_t *cond,
                          int32_t *need_kf, msl_mem out_mem) noexcept {
    try {
    return handle_form(WHO_KD, check_decision, launch_decision, h, n_frames, cap, lcap, pcap, n_tab, n_pts, n_lines, params, frames, depth, n_cur,
                       cur_held, outlier, cur_lheld, line_outlier, n_cur_lines, n_planes, pt_nobs, pt_flags, ln_nobs, held_id, n_kps, mem, plane_match,
                       plane_outlier, found_pt, found_line, n_inliers, track_ok, new_plane, held_out, outlier_out, lheld_out, line_outlier_out, counts,
                       cond, need_kf, out_mem);
    } MSL_ABI_CATCH_INT
}

int msl_keyframe_decision_batch(int device, int n_frames, int cap, int lcap, int pcap, int n_tab, int n_pts, int n_lines,
                                const msl_keyframe_params *params, const msl_keyframe_frame *frames, const float *depth, const int32_t *n_cur,
                                const int32_t *cur_held, const uint8_t *outlier, const int32_t *cur_lheld, const uint8_t *line_outlier,
                                const int32_t *n_cur_lines, const int32_t *n_planes, const int32_t *pt_nobs, const uint8_t *pt_flags,
                                const int32_t *ln_nobs, const int32_t *held_id, const int32_t *n_kps, msl_mem mem, int32_t *plane_match,
                                uint8_t *plane_outlier, uint8_t *found_pt, uint8_t *found_line, int32_t *n_inliers, uint8_t *track_ok,
                                uint8_t *new_plane, int32_t *held_out, uint8_t *outlier_out, int32_t *lheld_out, uint8_t *line_outlier_out,
                                int32_t *counts, uint8_t *cond, int32_t *need_kf, msl_mem out_mem) noexcept {
    try {
    return batch_form(check_decision, launch_decision, device, mem == MSL_MEM_DEVICE || out_mem == MSL_MEM_DEVICE, n_frames, cap, lcap, pcap, n_tab,
                      n_pts, n_lines, params, frames, depth, n_cur, cur_held, outlier, cur_lheld, line_outlier, n_cur_lines, n_planes, pt_nobs,
                      pt_flags, ln_nobs, held_id, n_kps, mem, plane_match, plane_outlier, found_pt, found_line, n_inliers, track_ok, new_plane,
                      held_out, outlier_out, lheld_out, line_outlier_out, counts, cond, need_kf, out_mem);
    } MSL_ABI_CATCH_INT
}

}  // extern "C"

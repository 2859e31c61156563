"""Sequential CPU models of the hand-over from tracking to local mapping, written statement by statement from the reference:

  points_3d            the point half of StereoInitialization (src/Tracking.cc:560-572), UpdateLastFrame (:1062-1104) and CreateNewKeyFrame
                       (:1524-1569) with Frame::UnprojectStereo (src/Frame.cc:515-526) and the two MapPoint constructors (src/MapPoint.cc:36-71):
                       what msl_points_3d computes for one frame
  keyframe_decision    the tail of TrackLocalMap (:1365-1430), mbNewPlane (:429-436), "Clean VO matches" (:450-465) and NeedNewKeyFrame
                       (:1433-1508) with KeyFrame::TrackedMapPoints (src/KeyFrame.cc:199-218): what msl_keyframe_decision computes for one frame
  walk_length_closed   the closed form of the walk's length the kernel uses; the model itself runs the loop with its break

Test infrastructure only.  Float conventions as tests/mappoint_model.py: float32 / float64 NumPy scalars wherever the
reference's type matters."""
import numpy as np

from tests import local_match_model as lm
from tests import mappoint_model as mm

F32, F64 = np.float32, np.float64
ALL, KEYFRAME, FRAME = 0, 1, 2
TRACKED_LOCAL_MAP, TRACK_OK, NEW_PLANE = 1, 2, 4
C1A, C1B, C1C, C2 = 1, 2, 4, 8
U32 = 1 << 32


def params(fx=517.3, fy=516.5, cx=318.6, cy=255.3, th_depth=3.0, min_points=100, nlevels=8, scale_factor=1.2):
    """msl_point3d_params as a dict; invfx / invfy as the library forms them."""
    p = mm.params(nlevels, scale_factor)
    p.update(fx=F32(fx), fy=F32(fy), cx=F32(cx), cy=F32(cy), th_depth=F32(th_depth), min_points=int(min_points))
    return p


def unproject_stereo(prm, u, v, z, Tcw):
    """Frame::UnprojectStereo for z > 0: (x3D, mOw)."""
    invfx, invfy = F32(1.0) / prm["fx"], F32(1.0) / prm["fy"]
    with np.errstate(all="ignore"):
        x = (F32(u) - prm["cx"]) * F32(z) * invfx                     # (u - cx) * z * invfx: float products, left to right
        y = (F32(v) - prm["cy"]) * F32(z) * invfy
        T = np.asarray(Tcw, F32).reshape(3, 4)
        Ow = lm.gemm3(T, True, -1.0, T[:, 3])                         # mOw = -mRcw.t() * mtcw
        return lm.gemm3(T, True, 1.0, np.array([x, y, F32(z)], F32), Ow), Ow   # mRwc * x3Dc + mOw


def frame_form_point(prm, X, Ow, octave):
    """MapPoint(Pos, pMap, pFrame, idxF) (src/MapPoint.cc:48-71): (normal, (min, max))."""
    with np.errstate(all="ignore"):
        v, nrm = mm.view_vector(Ow, X)                                # mNormalVector = mWorldPos - Ow; cv::norm
        inv = F64(1.0) / F64(nrm)
        normal = np.array([F32(F64(v[a]) * inv) for a in range(3)], F32)   # mNormalVector / cv::norm(mNormalVector): no 0 + x step
        dist = np.zeros(2, F32)
        if 0 <= octave < prm["nlevels"]:                              # pinned: an out-of-range read in the reference
            dmax = F32(nrm) * F32(prm["scale_factors"][octave])       # const float dist = cv::norm(PC); dist * levelScaleFactor
            dist[:] = dmax / F32(prm["scale_factors"][prm["nlevels"] - 1]), dmax
    return normal, dist


def keyframe_form_point(prm, X, Ow, octave):
    """MapPoint(Pos, pRefKF, pMap) + AddObservation + UpdateNormalAndDepth with the one observation: (normal, (min, max))."""
    if not 0 <= octave < prm["nlevels"]:                              # pinned as msl_refresh_map_points: nothing is written
        return np.zeros(3, F32), np.zeros(2, F32)
    return mm.normal_and_depth(prm, [Ow], Ow, octave, X)


def walk_length_closed(depth_members, th_depth, min_points):
    """min(M, max(#members with !(z > th_depth), min_points) + 1) for the members' depths."""
    M = len(depth_members)
    near = sum(1 for z in depth_members if not (F32(z) > F32(th_depth)))
    return min(M, max(near, min_points) + 1)


def walk(depth, mvpMapPoints, pt_nobs, mThDepth, min_points):
    """The loop CreateNewKeyFrame and UpdateLastFrame share, with its break: (the slots that get a point, in order; the slots whose held point
    is NULLed or overwritten; the final nPoints)."""
    vDepthIdx = []
    for i in range(len(depth)):
        z = F32(depth[i])
        if z > 0:
            vDepthIdx.append((float(z), i))
    vDepthIdx = sorted(vDepthIdx)                                      # sort of pair<float, int>
    created, cleared = [], []
    nPoints = 0
    for j in range(len(vDepthIdx)):
        i = vDepthIdx[j][1]
        bCreateNew = False
        pMP = mvpMapPoints[i]
        if pMP is None:
            bCreateNew = True
        elif pt_nobs[pMP] < 1:
            bCreateNew = True
            cleared.append(i)                                          # = NULL in CreateNewKeyFrame, overwritten in UpdateLastFrame
        if bCreateNew:
            created.append(i)                                          # new MapPoint(...)
            nPoints += 1
        else:
            nPoints += 1
        if F32(vDepthIdx[j][0]) > F32(mThDepth) and nPoints > min_points:
            break
    return created, cleared, nPoints


def points_3d(mode, prm, kps_un, depth, desc, Tcw, cur_held=None, pt_nobs=None, enable=True, first_id=None, cap=None):
    """msl_points_3d for one frame of n = len(depth) slots.  Returns the per-slot outputs as arrays of `cap` (default n) rows, new_order of cap
    entries, n_new, n_walked."""
    N = len(depth)
    cap = cap or max(N, 1)
    out = dict(pt_new=np.zeros(cap, np.uint8), cleared=np.zeros(cap, np.uint8), new_xyz=np.zeros((cap, 3), F32), new_normal=np.zeros((cap, 3), F32),
               new_dist=np.zeros((cap, 2), F32), new_desc=np.zeros((cap, 32), np.uint8), held_out=np.full(cap, -1, np.int32),
               new_order=np.full(cap, -1, np.int32), n_new=0, n_walked=0)
    n_pts = 0 if pt_nobs is None else len(pt_nobs)
    mvpMapPoints = [None] * N                                          # the slot's point id; ALL starts from an all-NULL frame
    if mode != ALL and cur_held is not None:
        out["held_out"][:N] = cur_held[:N]
        mvpMapPoints = [int(i) if 0 <= int(i) < n_pts else None for i in cur_held[:N]]   # an id outside the table counts as NULL
    if not enable:
        return out
    order = []

    def create(i):
        X, Ow = unproject_stereo(prm, kps_un["x"][i], kps_un["y"][i], depth[i], Tcw)
        form = frame_form_point if mode == FRAME else keyframe_form_point
        normal, dist = form(prm, X, Ow, int(kps_un["octave"][i]))
        out["pt_new"][i] = 1
        out["new_xyz"][i], out["new_normal"][i], out["new_dist"][i], out["new_desc"][i] = X, normal, dist, desc[i]
        out["held_out"][i] = -1 if first_id is None else first_id + len(order)
        order.append(i)

    if mode == ALL:
        for i in range(N):
            z = F32(depth[i])
            if z > 0:
                create(i)
                out["n_walked"] += 1
    else:
        created, cleared, out["n_walked"] = walk(depth[:N], mvpMapPoints, pt_nobs, prm["th_depth"], prm["min_points"])
        out["cleared"][cleared] = 1
        for i in created:
            create(i)
    out["n_new"] = len(order)
    out["new_order"][:len(order)] = order
    return out


def tracked_map_points(minObs, held_row, pt_flags, pt_nobs):
    """KeyFrame::TrackedMapPoints."""
    nPoints = 0
    bCheckObs = minObs > 0
    for pMP in held_row:
        pMP = int(pMP)
        if 0 <= pMP < len(pt_nobs):
            if pt_flags[pMP] & 1:
                if bCheckObs:
                    if pt_nobs[pMP] >= minObs:
                        nPoints += 1
                else:
                    nPoints += 1
    return nPoints


def keyframe_decision(prm, fr, table, pt_nobs, pt_flags, ln_nobs):
    """msl_keyframe_decision for one frame.  prm: dict(max_frames, min_frames, th_depth, only_tracking); fr: the record's fields and depth,
    cur_held, outlier, cur_lheld, line_outlier, plane_match (np, 3), plane_outlier (np, 3); table: the keyframes' held_id rows.  Returns the
    outputs, with plane_match / plane_outlier as they are left."""
    N, NL, NP = len(fr["depth"]), len(fr["cur_lheld"]), len(fr["plane_match"])
    n_pts, n_lines = len(pt_nobs), len(ln_nobs)
    point = lambda i: int(fr["cur_held"][i]) if 0 <= int(fr["cur_held"][i]) < n_pts else None
    line = lambda i: int(fr["cur_lheld"][i]) if 0 <= int(fr["cur_lheld"][i]) < n_lines else None
    mbOnlyTracking = bool(prm["only_tracking"])
    plane_match, plane_outlier = np.array(fr["plane_match"], np.int32).reshape(NP, 3), np.array(fr["plane_outlier"], np.uint8).reshape(NP, 3)
    found_pt, found_line = np.zeros(N, np.uint8), np.zeros(NL, np.uint8)
    mnId = int(fr["frame_id"]) % U32                                   # long unsigned int
    mnLastRelocFrameId, mnLastKeyFrameId = int(fr["last_reloc_frame_id"]) % U32, int(fr["last_keyframe_id"]) % U32   # unsigned int
    mMaxFrames, mMinFrames = int(prm["max_frames"]), int(prm["min_frames"])
    mbNewPlane = bool(fr["flags"] & NEW_PLANE)
    # ---- TrackLocalMap :1365-1430 ----
    if fr["flags"] & TRACKED_LOCAL_MAP:
        mbNewPlane = False                                             # PlaneMatcher::SearchMapByCoefficients (src/PlaneMatcher.cpp:32)
        mnMatchesInliers = 0
        for i in range(N):
            if point(i) is not None:
                if not fr["outlier"][i]:
                    found_pt[i] = 1
                    if not mbOnlyTracking:
                        if pt_nobs[point(i)] > 0:
                            mnMatchesInliers += 1
                    else:
                        mnMatchesInliers += 1
        for i in range(NL):
            if line(i) is not None:
                if not fr["line_outlier"][i]:
                    found_line[i] = 1
                    if not mbOnlyTracking:
                        if ln_nobs[line(i)] > 0:
                            mnMatchesInliers += 1
                    else:
                        mnMatchesInliers += 1
        for i in range(NP):
            if plane_match[i, 0] >= 0:
                if plane_outlier[i, 0]:
                    plane_match[i, 0] = -1
                else:
                    mnMatchesInliers += 1
            if plane_match[i, 1] >= 0:
                if plane_outlier[i, 1]:
                    plane_match[i, 1] = -1
                    plane_outlier[i, 1] = 0
            if plane_match[i, 2] >= 0:
                if plane_outlier[i, 2]:
                    plane_match[i, 2] = -1
                    plane_outlier[i, 2] = 0
        # unsigned int + int is unsigned int: the sum wraps at 2^32 before the comparison with the unsigned long mnId
        if mnId < (mnLastRelocFrameId + mMaxFrames) % U32 and mnMatchesInliers < 20:
            bOK = False
        elif mnMatchesInliers < 7:
            bOK = False
        else:
            bOK = True
    else:
        mnMatchesInliers = int(fr["n_inliers_in"])
        bOK = bool(fr["flags"] & TRACK_OK)
    # ---- :429-436 ----
    for i in range(NP):
        if plane_match[i, 0] >= 0:
            pass                                                       # UpdateCoefficientsAndPoints: msl_map_plane_merge
        elif not plane_outlier[i, 0]:
            mbNewPlane = True
    held_out, outlier_out = np.array(fr["cur_held"], np.int32), np.array(fr["outlier"], np.uint8)
    lheld_out, line_outlier_out = np.array(fr["cur_lheld"], np.int32), np.array(fr["line_outlier"], np.uint8)
    out = dict(found_pt=found_pt, found_line=found_line, n_inliers=mnMatchesInliers, track_ok=int(bOK), new_plane=int(mbNewPlane), held_out=held_out,
               outlier_out=outlier_out, lheld_out=lheld_out, line_outlier_out=line_outlier_out, counts=np.zeros(4, np.int32), cond=0, need_kf=0,
               plane_match=plane_match, plane_outlier=plane_outlier)
    if not bOK:
        return out
    # ---- Clean VO matches :450-465 ----
    for i in range(N):
        pMP = point(i)
        if pMP is not None:
            if pt_nobs[pMP] < 1:
                outlier_out[i] = 0
                held_out[i] = -1
    for i in range(NL):
        pML = line(i)
        if pML is not None:
            if ln_nobs[pML] < 1:
                line_outlier_out[i] = 0
                lheld_out[i] = -1
    # ---- NeedNewKeyFrame :1433-1508 ----
    if mbOnlyTracking:
        return out
    if fr["local_mapping_stopped"]:
        return out
    nKFs = int(fr["n_kfs"])
    if mnId < (mnLastRelocFrameId + mMaxFrames) % U32 and nKFs > mMaxFrames:
        return out
    nMinObs = 3
    if nKFs <= 2:
        nMinObs = 2
    ref = int(fr["ref_kf"])
    nRefMatches = tracked_map_points(nMinObs, table[ref], pt_flags, pt_nobs) if 0 <= ref < len(table) else 0   # pinned: no such keyframe
    bLocalMappingIdle = bool(fr["local_mapping_idle"])
    nMap = nTotal = nNonTrackedClose = 0
    for i in range(N):
        if F32(fr["depth"][i]) > 0 and F32(fr["depth"][i]) < F32(prm["th_depth"]):
            nTotal += 1
            if 0 <= held_out[i] < n_pts and not outlier_out[i]:
                nMap += 1
            else:
                nNonTrackedClose += 1
    ratioMap = F32(F64(F32(nMap)) / F64(max(1.0, float(nTotal))))      # (float)nMap / fmax(1.0f, nTotal): fmax's double overload, one rounding
    thRefRatio = F32(0.75)
    if nKFs < 2:
        thRefRatio = F32(0.4)
    thMapRatio = F32(0.35)
    if mnMatchesInliers > 300:
        thMapRatio = F32(0.20)
    c1a = mnId >= (mnLastKeyFrameId + mMaxFrames) % U32               # unsigned int + int, wrapping
    c1b = mnId >= (mnLastKeyFrameId + mMinFrames) % U32 and bLocalMappingIdle
    c1c = F64(mnMatchesInliers) < F64(nRefMatches) * F64(0.25) or ratioMap < F32(0.3)   # int * double: a double product
    c2 = (F32(mnMatchesInliers) < F32(nRefMatches) * thRefRatio or ratioMap < thMapRatio) and mnMatchesInliers > 15   # int * float: a float product
    out["counts"][:] = nRefMatches, nTotal, nMap, nNonTrackedClose
    out["cond"] = (C1A if c1a else 0) | (C1B if c1b else 0) | (C1C if c1c else 0) | (C2 if c2 else 0)
    if ((c1a or c1b or c1c) and c2) or mbNewPlane:
        if bLocalMappingIdle:
            out["need_kf"] = 1
        elif fr["keyframes_in_queue"] < 3:
            out["need_kf"] = 1
    return out

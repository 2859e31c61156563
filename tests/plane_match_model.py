"""A literal, sequential CPU model of PlaneMatcher::SearchMapByCoefficients (reference src/PlaneMatcher.cpp:31-106) with
Frame::ComputePlaneWorldCoeff (src/Frame.cc:656-660), the parity reference of msl_plane_associate[_batch].

Test infrastructure only.  Types as the reference has them: pM is a CV_32F cv::Mat product (cv::gemm's float kernel: double accumulation,
one rounding per element); angle a float dot product evaluated left to right; PointDistanceFromPlane a float expression whose absolute
value is compared as double against a running double that starts at 100; ldTh / lverTh / lparTh floats.  A frame is a dict of
manhattanslam_amd.plane (plane_coef, Tcw, plane_match, mp_w, mp_flags, mp_clouds).

search_prefix_scan is an independent formulation of the same loop (the three running thresholds as exclusive prefix minima / maxima)
used only to cross-check the literal one.  search_fast is the literal walk fed with distances and angles computed for all frame planes
at once in numpy float32 (the same left-to-right expressions): tests/test_plane_model.py asserts it equal to the literal one; it exists
for the scenes with 4096 map planes or millions of cloud points."""
import numpy as np

F32 = np.float32


def world_coef(Tcw, coef):
    """Frame::ComputePlaneWorldCoeff: mTcw^T * coef, mTcw's row 3 = 0 0 0 1 (:656-660)."""
    T = np.zeros((4, 4), F32)
    T[:3] = np.asarray(Tcw, F32).reshape(3, 4)
    T[3, 3] = 1
    out = np.zeros(4, F32)
    for r in range(4):
        s = 0.0
        for k in range(4):
            s += float(T[k, r]) * float(coef[k])
        out[r] = F32(s)
    return out


def point_distance_from_plane(pM, cloud):
    """PlaneMatcher::PointDistanceFromPlane (:95-106)."""
    res = 100.0
    for p in np.asarray(cloud, F32).reshape(-1, 3):
        dis = float(abs(pM[0] * p[0] + pM[1] * p[1] + pM[2] * p[2] + pM[3]))
        if dis < res:
            res = dis
    return res


def search_map_by_coefficients(fr, prm):
    """(nmatches, plane_match (K,3) i32 after the call, pM (K,4) f32).  prm: dict d_th, a_th, ver_th, par_th."""
    match = np.array(fr["plane_match"], np.int32, copy=True).reshape(-1, 3)
    K = len(fr["plane_coef"])
    pMs = np.zeros((K, 4), F32)
    nmatches = 0
    for i in range(K):                                                       # :36
        pM = world_coef(fr["Tcw"], fr["plane_coef"][i])                      # :38
        pMs[i] = pM
        ldTh, lverTh, lparTh = F32(prm["d_th"]), F32(prm["ver_th"]), F32(prm["par_th"])
        aTh = F32(prm["a_th"])
        found = False
        for j in range(len(fr["mp_w"])):                                     # :46
            if not (fr["mp_flags"][j] & 1):                                  # :47-50 isBad()
                continue
            pW = np.asarray(fr["mp_w"][j], F32)
            angle = pM[0] * pW[0] + pM[1] * pW[1] + pM[2] * pW[2]            # :54-56
            if angle > aTh:                                                  # :60
                dis = point_distance_from_plane(pM, fr["mp_clouds"][j])
                if dis < float(ldTh):
                    ldTh = F32(dis)
                    match[i, 0] = j
                    found = True
                    continue
            if angle < lverTh and angle > -lverTh:                           # :72-77
                lverTh = F32(abs(angle))
                match[i, 2] = j
                continue
            if angle > lparTh or angle < -lparTh:                            # :80-84
                lparTh = F32(abs(angle))
                match[i, 1] = j
        if found:
            nmatches += 1
    return nmatches, match, pMs


def pose_layout(match, mp_w):
    """plane_w (K,12) / plane_has (K,) as msl_plane_associate writes them: slot s holds an index in [0, M) -> bit s and the world position,
    else zeros."""
    K, M = len(match), len(mp_w)
    pw = np.zeros((K, 12), F32)
    ph = np.zeros(K, np.uint8)
    for k in range(K):
        for s in range(3):
            j = int(match[k, s])
            if 0 <= j < M:
                ph[k] |= 1 << s
                pw[k, 4 * s:4 * s + 4] = mp_w[j]
    return pw, ph


def search_prefix_scan(fr, prm):
    """The same result by exclusive prefix scans over the map planes, vectorised (no sequential threshold state)."""
    match = np.array(fr["plane_match"], np.int32, copy=True).reshape(-1, 3)
    M = len(fr["mp_w"])
    nmatches = 0
    if M == 0:
        return nmatches, match, np.array([world_coef(fr["Tcw"], c) for c in fr["plane_coef"]], F32).reshape(-1, 4)
    W = np.asarray(fr["mp_w"], F32).reshape(M, 4)
    good = (np.asarray(fr["mp_flags"]) & 1).astype(bool)
    pMs = []
    for i in range(len(fr["plane_coef"])):
        pM = world_coef(fr["Tcw"], fr["plane_coef"][i])
        pMs.append(pM)
        angle = (pM[0] * W[:, 0] + pM[1] * W[:, 1]) + pM[2] * W[:, 2]
        dis = np.full(M, 100.0)
        for j in range(M):
            c = np.asarray(fr["mp_clouds"][j], F32).reshape(-1, 3)
            d = np.abs(((pM[0] * c[:, 0] + pM[1] * c[:, 1]) + pM[2] * c[:, 2]) + pM[3]).astype(np.float64)
            d = d[~np.isnan(d)]
            dis[j] = min(100.0, d.min()) if len(d) else 100.0
        A = good & (angle > F32(prm["a_th"]))
        run = np.minimum.accumulate(np.where(A, dis, np.inf))
        before = np.concatenate([[float(F32(prm["d_th"]))], np.minimum(float(F32(prm["d_th"])), run[:-1])])
        hit = A & (dis < before)
        aa = np.abs(angle).astype(np.float64)
        rest = good & ~hit & ~np.isnan(angle)
        runv = np.minimum.accumulate(np.where(rest, aa, np.inf))
        bv = np.concatenate([[float(F32(prm["ver_th"]))], np.minimum(float(F32(prm["ver_th"])), runv[:-1])])
        ver = rest & (aa < bv)
        rp = rest & ~ver
        runp = np.maximum.accumulate(np.where(rp, aa, -np.inf))
        bp = np.concatenate([[float(F32(prm["par_th"]))], np.maximum(float(F32(prm["par_th"])), runp[:-1])])
        par = rp & (aa > bp)
        for s, sel in ((0, hit), (1, par), (2, ver)):
            if sel.any():
                match[i, s] = np.flatnonzero(sel)[-1]
        nmatches += int(hit.any())
    return nmatches, match, np.array(pMs, F32).reshape(-1, 4)


def cloud_distances(pMs, cloud):
    """point_distance_from_plane of every row of pMs (K,4) f32 against one cloud, vectorised: (K,) float64."""
    c = np.asarray(cloud, F32).reshape(-1, 3)
    out = np.full(len(pMs), 100.0)
    if len(c) == 0:
        return out
    with np.errstate(invalid="ignore", over="ignore"):
        for k0 in range(0, len(pMs), max(1, (1 << 22) // len(c))):           # blocks of frame planes, to bound the temporaries
            p = pMs[k0:k0 + max(1, (1 << 22) // len(c))]
            d = np.abs(((p[:, 0:1] * c[:, 0] + p[:, 1:2] * c[:, 1]) + p[:, 2:3] * c[:, 2]) + p[:, 3:4])
            m = np.fmin.reduce(d, axis=1)                                    # NaN distances never replace the minimum
            out[k0:k0 + len(p)] = np.where(m < 100.0, m, 100.0)
    return out


def search_fast(fr, prm):
    """search_map_by_coefficients with the distances and angles precomputed; the walk itself is the literal one."""
    match = np.array(fr["plane_match"], np.int32, copy=True).reshape(-1, 3)
    K, M = len(fr["plane_coef"]), len(fr["mp_w"])
    pMs = np.array([world_coef(fr["Tcw"], c) for c in fr["plane_coef"]], F32).reshape(-1, 4)
    if K == 0 or M == 0:
        return 0, match, pMs
    W = np.asarray(fr["mp_w"], F32).reshape(M, 4)
    good = [bool(x & 1) for x in np.asarray(fr["mp_flags"]).tolist()]
    with np.errstate(invalid="ignore", over="ignore"):
        ang = (pMs[:, None, 0] * W[None, :, 0] + pMs[:, None, 1] * W[None, :, 1]) + pMs[:, None, 2] * W[None, :, 2]
    aTh = float(F32(prm["a_th"]))
    dis = np.full((K, M), 100.0)
    need = np.flatnonzero((ang > F32(prm["a_th"])).any(0) & np.array(good))
    for j in need:
        dis[:, j] = cloud_distances(pMs, fr["mp_clouds"][j])
    ang, dis = ang.astype(np.float64).tolist(), dis.tolist()                  # floats widen exactly
    nmatches = 0
    for i in range(K):
        ldTh, lverTh, lparTh = float(F32(prm["d_th"])), float(F32(prm["ver_th"])), float(F32(prm["par_th"]))
        found = False
        ai, di = ang[i], dis[i]
        for j in range(M):
            if not good[j]:
                continue
            angle = ai[j]
            if angle > aTh:
                if di[j] < ldTh:
                    ldTh = di[j]
                    match[i, 0] = j
                    found = True
                    continue
            if angle < lverTh and angle > -lverTh:
                lverTh = abs(angle)
                match[i, 2] = j
                continue
            if angle > lparTh or angle < -lparTh:
                lparTh = abs(angle)
                match[i, 1] = j
        nmatches += found
    return nmatches, match, pMs

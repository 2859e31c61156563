"""A literal, sequential CPU model of Tracking::SearchLocalPoints after its first loop (reference src/Tracking.cc:1654-1695):
Frame::isInFrustum (src/Frame.cc:204-259) with MapPoint::PredictScale (src/MapPoint.cc:350-364) for every candidate local map point,
then ORBmatcher::SearchByProjection(Frame &F, const vector<MapPoint*> &vpMapPoints, th) (src/ORBmatcher.cc:40-117) with
RadiusByViewingCos (:119-124) and Frame::GetFeaturesInArea (src/Frame.cc:332-381).

Test infrastructure only.  Float conventions are the ones DESIGN.md section 3 pins for the kernels: float32 scalars everywhere, the 3x3
cv::Mat products as cv::gemm's float kernel (double accumulation, one rounding), cv::norm / Mat::dot as double sums of double products,
log as the double log of the float rounded once.  Inputs are the dicts of manhattanslam_amd.match.pack_local_points."""
import math

import numpy as np

F32 = np.float32
TH_HIGH = 100                     # src/ORBmatcher.cc:33
GRID_COLS, GRID_ROWS = 64, 48     # FRAME_GRID_COLS / ROWS


def gemm3(T, transA, alpha, b, c=None):
    """cv::gemm's CV_32F kernel for a 3x3 block of the row-major 3x4 T times a 3-vector: double accumulation, one rounding."""
    out = np.zeros(3, F32)
    for r in range(3):
        s = 0.0
        for k in range(3):
            a = T[k, r] if transA else T[r, k]
            s += float(a) * float(b[k])
        out[r] = F32(s * alpha + (float(c[r]) if c is not None else 0.0))
    return out


def predict_scale(max_distance, dist, log_scale, nlevels):
    """MapPoint::PredictScale (src/MapPoint.cc:350-364).  A non-finite / out-of-int quotient converts to INT_MIN (x86-64) -> level 0."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ratio = F32(max_distance) / F32(dist)
        r = float(ratio)
        lg = F32(math.log(r)) if r > 0 and math.isfinite(r) else (F32(np.inf) if r == math.inf else (F32(-np.inf) if r == 0 else F32(np.nan)))
        q = np.ceil(lg / F32(log_scale))
    n = int(q) if (math.isfinite(float(q)) and -2147483648.0 <= float(q) < 2147483648.0) else -2147483648
    return 0 if n < 0 else (nlevels - 1 if n >= nlevels else n)


def is_in_frustum(p, T, xyz, normal, dmin, dmax, view_cos_limit, log_scale):
    """Frame::isInFrustum (src/Frame.cc:204-259): None, or (u, v, u - mbf * invz, level, viewCos)."""
    fx, fy, cx, cy, bf = (F32(p[k]) for k in ("fx", "fy", "cx", "cy", "bf"))
    minX, maxX, minY, maxY = (F32(p[k]) for k in ("minX", "maxX", "minY", "maxY"))
    tcw = T[:, 3]
    P = np.asarray(xyz, F32)
    Pc = gemm3(T, False, 1.0, P, tcw)                              # :211  mRcw * P + mtcw
    PcX, PcY, PcZ = Pc
    if PcZ < F32(0):                                                # :217
        return None
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        invz = F32(1) / PcZ                                         # :221
        u = fx * PcX * invz + cx                                    # :222, left to right
        v = fy * PcY * invz + cy
    if u < minX or u > maxX:                                        # :225 (a NaN passes)
        return None
    if v < minY or v > maxY:
        return None
    maxDistance = F32(1.2) * F32(dmax)                              # GetMaxDistanceInvariance
    minDistance = F32(0.8) * F32(dmin)
    Ow = gemm3(T, True, -1.0, tcw)                                  # Frame::UpdatePoseMatrices: mOw = -mRcw.t() * mtcw
    PO = P - Ow                                                     # :233, float32
    dist = F32(math.sqrt(sum(float(PO[k]) * float(PO[k]) for k in range(3))))   # :234 cv::norm
    if dist < minDistance or dist > maxDistance:                    # :236
        return None
    Pn = np.asarray(normal, F32)
    dot = 0.0
    for k in range(3):
        dot += float(PO[k]) * float(Pn[k])                          # Mat::dot
    viewCos = F32(dot / float(dist))                                # :242
    if viewCos < F32(view_cos_limit):                               # :244
        return None
    level = predict_scale(dmax, dist, log_scale, int(p["nlevels"]))  # :248
    with np.errstate(invalid="ignore", over="ignore"):
        xr = u - bf * invz                                          # :253
    return u, v, xr, level, viewCos


def radius_by_viewing_cos(view_cos):
    """ORBmatcher::RadiusByViewingCos (src/ORBmatcher.cc:119-124): float compared with a double constant."""
    return F32(2.5) if float(view_cos) > 0.998 else F32(4.0)


def features_in_area(p, grid, kps, un_xy, x, y, r, min_level, max_level):
    """Frame::GetFeaturesInArea (src/Frame.cc:332-381); grid: cell id (ix * 48 + iy) -> keypoint indices in insertion order."""
    minX, maxX, minY, maxY = (F32(p[k]) for k in ("minX", "maxX", "minY", "maxY"))
    wInv = F32(GRID_COLS) / (maxX - minX)
    hInv = F32(GRID_ROWS) / (maxY - minY)
    x, y, r = F32(x), F32(y), F32(r)
    if math.isnan(float(x)) or math.isnan(float(y)):               # (int)floor(NaN) is INT_MIN on x86-64: nMaxCell < 0, empty
        return []
    x0 = max(0, int(np.floor((x - minX - r) * wInv)))
    if x0 >= GRID_COLS:
        return []
    x1 = min(GRID_COLS - 1, int(np.ceil((x - minX + r) * wInv)))
    if x1 < 0:
        return []
    y0 = max(0, int(np.floor((y - minY - r) * hInv)))
    if y0 >= GRID_ROWS:
        return []
    y1 = min(GRID_ROWS - 1, int(np.ceil((y - minY + r) * hInv)))
    if y1 < 0:
        return []
    bCheckLevels = min_level > 0 or max_level >= 0
    out = []
    for ix in range(x0, x1 + 1):
        for iy in range(y0, y1 + 1):
            for i in grid.get(ix * GRID_ROWS + iy, ()):
                octave = int(kps["octave"][i])
                if bCheckLevels:
                    if octave < min_level:
                        continue
                    if max_level >= 0 and octave > max_level:
                        continue
                distx = F32(un_xy[i, 0]) - x
                disty = F32(un_xy[i, 1]) - y
                if abs(distx) < r and abs(disty) < r:
                    out.append(i)
    return out


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def search_local_points(p, cur, local, T):
    """One frame.  p: a LOCAL_MATCH_PARAMS_DTYPE record; cur / local: the per-frame dicts of pack_local_points; T: 3x4 or 4x4 mTcw.
    Returns (match (N,) i32, n_to_match, nmatches, in_view (M,) u8, track (M,) LOCAL_TRACK_DTYPE) -- what msl_match_local_points reports."""
    from manhattanslam_amd import LOCAL_TRACK_DTYPE
    p = p.reshape(-1)[0] if isinstance(p, np.ndarray) and p.shape else p
    T = np.asarray(T, F32)[:3, :4]
    n, m = len(cur["kps"]), len(local["xyz"])
    th = F32(p["th"])
    scale = p["scale_factors"].astype(F32)
    # the second loop of SearchLocalPoints (:1670-1684)
    in_view = np.zeros(m, np.uint8)
    track = np.zeros(m, LOCAL_TRACK_DTYPE)
    n_to_match = 0
    for j in range(m):
        if not (local["flags"][j] & 1):                             # mnLastFrameSeen == current id, or isBad()
            continue
        res = is_in_frustum(p, T, local["xyz"][j], local["normal"][j], local["dist"][j][0], local["dist"][j][1], p["view_cos_limit"],
                            p["log_scale_factor"])
        if res is None:
            continue
        u, v, xr, level, vc = res
        in_view[j] = 1
        track[j] = (u, v, xr, level, vc)
        n_to_match += 1
    # F.mvpMapPoints as SearchByProjection sees it: holder (-2 = the point held on entry, j = local point written here) and its Observations() > 0
    holder = [-2 if (cur["flags"][i] & 1) else -1 for i in range(n)]
    holder_obs = [bool(cur["flags"][i] & 1) and bool(cur["flags"][i] & 2) for i in range(n)]
    grid = {}
    for i in range(n):
        c = int(cur["grid_cell"][i])
        if c >= 0:
            grid.setdefault(c, []).append(i)
    nmatches = 0
    nn_ratio = F32(p["nn_ratio"])
    if n_to_match > 0:                                              # :1686
        for j in range(m):                                          # src/ORBmatcher.cc:45-113
            if not in_view[j]:
                continue
            L = int(track["scale_level"][j])
            r = radius_by_viewing_cos(track["view_cos"][j])
            if th != F32(1.0):
                r = r * th
            rs = r * scale[L]
            idxs = features_in_area(p, grid, cur["kps"], cur["un_xy"], track["proj_x"][j], track["proj_y"][j], rs, L - 1, L)
            if not idxs:
                continue
            bestDist, bestLevel, bestDist2, bestLevel2, bestIdx = 256, -1, 256, -1, -1
            for idx in idxs:
                if holder[idx] != -1 and holder_obs[idx]:           # :81-83
                    continue
                if F32(cur["uright"][idx]) > F32(0):                # :84-88
                    er = abs(F32(track["proj_xr"][j]) - F32(cur["uright"][idx]))
                    if er > rs:
                        continue
                dist = hamming(local["desc"][j], cur["desc"][idx])
                if dist < bestDist:                                 # :94-103
                    bestDist2, bestDist = bestDist, dist
                    bestLevel2, bestLevel = bestLevel, int(cur["kps"]["octave"][idx])
                    bestIdx = idx
                elif dist < bestDist2:
                    bestLevel2 = int(cur["kps"]["octave"][idx])
                    bestDist2 = dist
            if bestDist <= TH_HIGH:                                 # :106-112
                if bestLevel == bestLevel2 and F32(bestDist) > nn_ratio * F32(bestDist2):
                    continue
                holder[bestIdx] = j
                holder_obs[bestIdx] = bool(local["flags"][j] & 2)
                nmatches += 1
    match = np.array([h if h >= 0 else -1 for h in holder], np.int32)
    return match, n_to_match, nmatches, in_view, track

"""Sequential model of msl_triangulate_new_points: LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:303-522) with
ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:257-406), CheckDistEpipolarLine (:127-144), LocalMapping::ComputeF12 (:624-640),
KeyFrame::UnprojectStereo and, for the new two-observation point, MapPoint::UpdateNormalAndDepth -- the literal restatement: neighbours in
order, AddMapPoint as an update of KF1's held flags, the two FeatureVectors merged as the reference merges them, every idx1 of a node
against every idx2 of the node in list order.  It is deliberately NOT the parallel decomposition of the kernels.

Pins: cv::Mat products accumulate in double and round once (gemm); Mat::dot / cv::norm accumulate in double; K.inv()
by the closed 3x3 form in double; comparisons against double literals in double; cos(2 atan2(b / 2, d)) = (d^2 - a^2) / (d^2 + a^2) in
double; cv::SVD = the Jacobi eigen-solver of tests/pnp_model.py on A^T A (double, n = 4), vt.row(3) = the eigenvector of the smallest
eigenvalue cast to float, then a float division; UnprojectStereo with depth <= 0 = low parallax; a keypoint whose octave is outside
[0, nlevels) is never searched.  NumPy float32 / float64 element-wise arithmetic only (+ - * / sqrt): it rounds as the scalar operation."""
import bisect

import numpy as np

from tests.pnp_model import jacobi_eig

F32, F64 = np.float32, np.float64
TH_LOW, HISTO_LENGTH = 50, 30
(NO_MATCH, TRIANGULATED, STEREO1, STEREO2, NEIGHBOUR_SKIPPED, LOW_PARALLAX, W_ZERO, Z1, Z2, REPROJ1, REPROJ2, ZERO_DIST, SCALE) = range(13)
CREATED = (TRIANGULATED, STEREO1, STEREO2)
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


# ---- cv::Mat arithmetic ---------------------------------------------------------------------------------------------------------------------
def gemm(A, B, alpha=1.0, C=None):
    """(float)(alpha * sum_k A[.., r, k] B[.., k, c] + C) with the products accumulated in double in k order; A (.., m, 3), B (.., 3, n)."""
    A = np.asarray(A, F32).astype(F64); B = np.asarray(B, F32).astype(F64)
    s = np.zeros(np.broadcast_shapes(A.shape[:-2], B.shape[:-2]) + (A.shape[-2], B.shape[-1]), F64)
    for k in range(A.shape[-1]):
        s = s + A[..., :, k, None] * B[..., None, k, :]
    return (s * F64(alpha) + (F64(0.0) if C is None else np.asarray(C, F32).astype(F64))).astype(F32)


def mv(A, v, alpha=1.0, c=None):
    """gemm of a matrix (.., 3, 3) and a column vector (.., 3) (+ c)."""
    return gemm(A, np.asarray(v, F32)[..., None], alpha, None if c is None else np.asarray(c, F32)[..., None])[..., 0]


def dot(a, b):
    """Mat::dot: double accumulation in index order (a double)."""
    a = np.asarray(a, F32).astype(F64); b = np.asarray(b, F32).astype(F64)
    s = np.zeros(np.broadcast_shapes(a.shape, b.shape)[:-1], F64)
    for k in range(a.shape[-1]):
        s = s + a[..., k] * b[..., k]
    return s


def norm(a):
    """cv::norm (a double)."""
    return np.sqrt(dot(a, a))


def inv3(M):
    """cv::invert of a 3x3 float matrix: the closed form, determinant and cofactors in double, times 1 / det, each element rounded."""
    m = np.asarray(M, F32).astype(F64)
    d = m[0, 0] * (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) - m[0, 1] * (m[1, 0] * m[2, 2] - m[1, 2] * m[2, 0]) + m[0, 2] * (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0])
    d = F64(1.0) / d
    t = [(m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) * d, (m[0, 2] * m[2, 1] - m[0, 1] * m[2, 2]) * d, (m[0, 1] * m[1, 2] - m[0, 2] * m[1, 1]) * d,
         (m[1, 2] * m[2, 0] - m[1, 0] * m[2, 2]) * d, (m[0, 0] * m[2, 2] - m[0, 2] * m[2, 0]) * d, (m[0, 2] * m[1, 0] - m[0, 0] * m[1, 2]) * d,
         (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]) * d, (m[0, 1] * m[2, 0] - m[0, 0] * m[2, 1]) * d, (m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]) * d]
    return np.array(t, F64).astype(F32).reshape(3, 3)


def params(fx, fy, cx, cy, bf, nlevels=8, scale_factor=1.2, check_orientation=False, only_stereo=False):
    """The camera and scale tables as the reference's ORBextractor / KeyFrame form them (float)."""
    sf = np.ones(nlevels, F32)
    for i in range(1, nlevels):
        sf[i] = sf[i - 1] * F32(scale_factor)
    return dict(fx=F32(fx), fy=F32(fy), cx=F32(cx), cy=F32(cy), invfx=F32(1.0) / F32(fx), invfy=F32(1.0) / F32(fy), bf=F32(bf), b=F32(bf) / F32(fx),
                nlevels=nlevels, scale_factors=sf, level_sigma2=sf * sf, scale_factor=F32(scale_factor), check_orientation=bool(check_orientation),
                only_stereo=bool(only_stereo))


# ---- poses and the pair geometry ------------------------------------------------------------------------------------------------------------
def pose(Tcw):
    """KeyFrame::SetPose: Rcw, tcw, Rwc, Ow = -Rwc * tcw."""
    T = np.asarray(Tcw, F32).reshape(3, 4)
    R, t = T[:, :3].copy(), T[:, 3].copy()
    return dict(T=T, Rcw=R, tcw=t, Rwc=R.T.copy(), Ow=mv(R.T, t, -1.0))


def rot_bin(rot):
    rot = F32(rot)
    if rot < 0.0:
        rot = rot + F32(360.0)
    b = int(np.floor(F64(rot * (F32(1.0) / F32(HISTO_LENGTH))) + 0.5)) if rot >= 0 else -1    # round() of a non-negative float: half away = half up
    if b == HISTO_LENGTH:
        b = 0
    return b if 0 <= b < HISTO_LENGTH else -1


def three_maxima(hist):
    """ORBmatcher::ComputeThreeMaxima on the bin counts."""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(hist):
        if s > max1:
            max3, max2, max1 = max2, max1, s; ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s; ind3, ind2 = ind2, i
        elif s > max3:
            max3 = s; ind3 = i
    if F32(max2) < F32(0.1) * F32(max1):
        ind2 = ind3 = -1
    elif F32(max3) < F32(0.1) * F32(max1):
        ind3 = -1
    return (ind1, ind2, ind3), (max1, max2, max3)


def pair_geometry(prm, T1, T2, margins=None):
    """The baseline, ComputeF12 and the epipole of SearchForTriangulation for (KF1, KF2)."""
    p1, p2 = pose(T1), pose(T2)
    baseline = F32(norm(p2["Ow"] - p1["Ow"]))
    if margins is not None:
        margins.append(("baseline", float(baseline), float(prm["b"]), float(prm["b"])))
    R12 = gemm(p1["Rcw"], p2["Rcw"].T)
    M = gemm(p1["Rcw"], p2["Rcw"].T, -1.0)
    t12 = mv(M, p2["tcw"], 1.0, p1["tcw"])
    z = F32(0.0)
    t12x = np.array([[z, -t12[2], t12[1]], [t12[2], z, -t12[0]], [-t12[1], t12[0], z]], F32)
    K = np.array([[prm["fx"], 0, prm["cx"]], [0, prm["fy"], prm["cy"]], [0, 0, 1]], F32)
    F12 = gemm(gemm(gemm(inv3(K.T), t12x), R12), inv3(K))
    C2 = mv(p2["Rcw"], p1["Ow"], 1.0, p2["tcw"])
    with np.errstate(all="ignore"):
        invz = F32(1.0) / C2[2]
        ex = prm["fx"] * C2[0] * invz + prm["cx"]
        ey = prm["fy"] * C2[1] * invz + prm["cy"]
    return dict(p1=p1, p2=p2, baseline=baseline, skip=bool(baseline < prm["b"]), F12=F12, ex=F32(ex), ey=F32(ey))


# ---- SearchForTriangulation -----------------------------------------------------------------------------------------------------------------
def feature_vector(kf):
    """DBoW2::FeatureVector: node -> the features of the node in ascending order (node -1: in no list)."""
    fv = {}
    for i, nd in enumerate(kf["node"]):
        if nd >= 0:
            fv.setdefault(int(nd), []).append(i)
    return fv


def search_for_triangulation(prm, kf1, kf2, geo, held1, trace=None, margins=None):
    """vMatches12 (-1 = none) after the rotation cull, the return value, and the bin of every match before the cull.  held1: KF1's
    GetMapPoint(i) != NULL as it is when this neighbour is searched."""
    n1 = len(kf1["kps_un"])
    F = geo["F12"]
    ex, ey = geo["ex"], geo["ey"]
    sf, sig2, nl = prm["scale_factors"], prm["level_sigma2"], prm["nlevels"]
    match = np.full(n1, -1, np.int64)
    bins = np.full(n1, -1, np.int64)
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    fv1, fv2 = feature_vector(kf1), feature_vector(kf2)
    k1, k2 = sorted(fv1), sorted(fv2)
    oct_ok1 = (kf1["kps_un"]["octave"] >= 0) & (kf1["kps_un"]["octave"] < nl)
    oct_ok2 = (kf2["kps_un"]["octave"] >= 0) & (kf2["kps_un"]["octave"] < nl)
    x2a, y2a, o2a = kf2["kps_un"]["x"], kf2["kps_un"]["y"], np.clip(kf2["kps_un"]["octave"], 0, nl - 1)
    i = j = 0
    while i < len(k1) and j < len(k2):
        if k1[i] == k2[j]:
            l1, l2 = fv1[k1[i]], np.array(fv2[k2[j]], np.int64)
            skip2 = (kf2["held"][l2] != 0) | ~oct_ok2[l2]
            st2 = kf2["uright"][l2] >= 0
            if prm["only_stereo"]:
                skip2 |= ~st2
            x2, y2, o2 = x2a[l2], y2a[l2], o2a[l2]
            with np.errstate(all="ignore"):
                distex, distey = ex - x2, ey - y2
                epi_lhs = distex * distex + distey * distey
                epi_rhs = F32(100) * sf[o2]
            for idx1 in l1:
                if held1[idx1] or not oct_ok1[idx1]:
                    continue
                stereo1 = kf1["uright"][idx1] >= 0
                if prm["only_stereo"] and not stereo1:
                    continue
                kp1 = kf1["kps_un"][idx1]
                dist = _POP[kf1["desc"][idx1][None, :] ^ kf2["desc"][l2]].sum(1)
                # CheckDistEpipolarLine for the whole list
                a = kp1["x"] * F[0, 0] + kp1["y"] * F[1, 0] + F[2, 0]
                b = kp1["x"] * F[0, 1] + kp1["y"] * F[1, 1] + F[2, 1]
                c = kp1["x"] * F[0, 2] + kp1["y"] * F[1, 2] + F[2, 2]
                num = a * x2 + b * y2 + c
                den = a * a + b * b
                with np.errstate(all="ignore"):
                    dsqr = num * num / den
                line_ok = (dsqr.astype(F64) < 3.84 * sig2[o2].astype(F64)) if den != 0 else np.zeros(len(l2), bool)
                best_dist, best_idx2 = TH_LOW, -1
                for q in range(len(l2)):
                    if skip2[q]:
                        continue
                    d = int(dist[q])
                    if d > TH_LOW or d > best_dist:
                        continue
                    if trace is not None and d == best_dist and best_idx2 >= 0 and line_ok[q] and not (not stereo1 and not st2[q] and epi_lhs[q] < epi_rhs[q]):
                        trace["ties"].append((idx1, best_idx2, int(l2[q])))
                    if not stereo1 and not st2[q]:
                        if epi_lhs[q] < epi_rhs[q]:
                            if trace is not None:
                                trace["epipole_rejects"].append((idx1, int(l2[q])))
                            continue
                    if line_ok[q]:
                        best_idx2, best_dist = int(l2[q]), d
                if margins is not None:
                    for q in np.nonzero(~skip2 & (dist <= TH_LOW))[0]:
                        if not stereo1 and not st2[q]:
                            margins.append(("epipole", float(epi_lhs[q]), float(epi_rhs[q]), float(epi_rhs[q])))
                        margins.append(("epiline", float(dsqr[q]), 3.84 * float(sig2[o2[q]]), 3.84 * float(sig2[o2[q]])))
                if best_idx2 >= 0:
                    match[idx1] = best_idx2
                    nmatches += 1
                    bins[idx1] = rot_bin(kp1["angle"] - kf2["kps_un"]["angle"][best_idx2])
                    if prm["check_orientation"] and bins[idx1] >= 0:
                        rot_hist[bins[idx1]].append(idx1)
            i += 1; j += 1
        elif k1[i] < k2[j]:
            i = bisect.bisect_left(k1, k2[j])
        else:
            j = bisect.bisect_left(k2, k1[i])
    before = match.copy()
    keep = (-1, -1, -1)
    if prm["check_orientation"]:
        keep, maxes = three_maxima([len(h) for h in rot_hist])
        if margins is not None and maxes[0] > 0:
            margins.append(("maxima2", float(maxes[1]), 0.1 * maxes[0], float(maxes[0])))
            margins.append(("maxima3", float(maxes[2]), 0.1 * maxes[0], float(maxes[0])))
        for b in range(HISTO_LENGTH):
            if b in keep:
                continue
            for idx1 in rot_hist[b]:
                match[idx1] = -1
                nmatches -= 1
    return match, nmatches, dict(before=before, bins=bins, keep=keep)


# ---- the triangulation loop, for all matched pairs of one neighbour at once ------------------------------------------------------------------
def cos_stereo(b, depth):
    a = (F32(b) / F32(2)).astype(F64) if isinstance(b, np.ndarray) else F64(F32(b) / F32(2))
    d = np.asarray(depth, F32).astype(F64)
    with np.errstate(all="ignore"):
        return ((d * d - a * a) / (d * d + a * a)).astype(F32)


def null_vector(A):
    """vt.row(3) of cv::SVD of the float A (.., 4, 4), pinned: the eigenvector of the smallest eigenvalue of A^T A, cast to float."""
    A64 = np.asarray(A, F32).astype(F64)
    G = np.zeros(A64.shape, F64)
    for k in range(4):
        G = G + A64[..., k, :, None] * A64[..., k, None, :]
    _, ut = jacobi_eig(G)
    return ut[..., 3, :].astype(F32)


def unproject_stereo(prm, p, raw_xy, depth):
    z = np.asarray(depth, F32)
    x = (raw_xy[..., 0] - prm["cx"]) * z * prm["invfx"]
    y = (raw_xy[..., 1] - prm["cy"]) * z * prm["invfy"]
    return mv(p["Rwc"], np.stack([x, y, z], -1), 1.0, p["Ow"])


def _reproj_bad(prm, p, X, z, kp, ur, stereo, margins, name):
    sig2 = prm["level_sigma2"][np.clip(kp["octave"], 0, prm["nlevels"] - 1)]
    with np.errstate(all="ignore"):
        x = (dot(p["Rcw"][0], X) + F64(p["tcw"][0])).astype(F32)
        y = (dot(p["Rcw"][1], X) + F64(p["tcw"][1])).astype(F32)
        invz = (F64(1.0) / z.astype(F64)).astype(F32)
        u = prm["fx"] * x * invz + prm["cx"]
        v = prm["fy"] * y * invz + prm["cy"]
        ex, ey = u - kp["x"], v - kp["y"]
        u_r = u - prm["bf"] * invz
        exr = u_r - ur
        e_mono = ex * ex + ey * ey
        e_st = ex * ex + ey * ey + exr * exr
    err = np.where(stereo, e_st, e_mono).astype(F64)
    th = np.where(stereo, 7.8, 5.991) * sig2.astype(F64)
    return err > th, err, th


def verdicts(prm, kf1, kf2, geo, idx1, idx2, margins=None):
    """The triangulation loop body for the pairs (idx1[k], idx2[k]): status and, where a point is created, the point."""
    idx1 = np.asarray(idx1, np.int64); idx2 = np.asarray(idx2, np.int64)
    N = len(idx1)
    out = dict(status=np.zeros(N, np.int64), xyz=np.zeros((N, 3), F32), normal=np.zeros((N, 3), F32), dist=np.zeros((N, 2), F32),
               cos=np.zeros((N, 3), F32), x3d=np.zeros((N, 4), F32))
    if N == 0:
        out.update(X_all=np.zeros((0, 3), F32), A=np.zeros((0, 4, 4), F32), tri=np.zeros(0, bool))
        return out
    p1, p2 = geo["p1"], geo["p2"]
    kp1, kp2 = kf1["kps_un"][idx1], kf2["kps_un"][idx2]
    ur1, ur2 = kf1["uright"][idx1], kf2["uright"][idx2]
    s1, s2 = ur1 >= 0, ur2 >= 0
    one = np.ones(N, F32)
    xn1 = np.stack([(kp1["x"] - prm["cx"]) * prm["invfx"], (kp1["y"] - prm["cy"]) * prm["invfy"], one], -1)
    xn2 = np.stack([(kp2["x"] - prm["cx"]) * prm["invfx"], (kp2["y"] - prm["cy"]) * prm["invfy"], one], -1)
    ray1, ray2 = mv(p1["Rwc"], xn1), mv(p2["Rwc"], xn2)
    with np.errstate(all="ignore"):
        cos_rays = (dot(ray1, ray2) / (norm(ray1) * norm(ray2))).astype(F32)
        plus1 = cos_rays + F32(1)
        cos1 = np.where(s1, cos_stereo(prm["b"], kf1["depth"][idx1]), plus1)
        cos2 = np.where(~s1 & s2, cos_stereo(prm["b"], kf2["depth"][idx2]), plus1)
        cos_st = np.where(cos2 < cos1, cos2, cos1)
        tri = (cos_rays < cos_st) & (cos_rays > 0) & (s1 | s2 | (cos_rays.astype(F64) < 0.9998))
        T1, T2 = p1["T"], p2["T"]
        A = np.stack([xn1[:, 0, None] * T1[2][None] - T1[0][None], xn1[:, 1, None] * T1[2][None] - T1[1][None],
                      xn2[:, 0, None] * T2[2][None] - T2[0][None], xn2[:, 1, None] * T2[2][None] - T2[1][None]], 1).astype(F32)
        x4 = null_vector(A)
        Xt = x4[:, :3] / x4[:, 3:4]
        d1, d2 = kf1["depth"][idx1], kf2["depth"][idx2]
        X1 = unproject_stereo(prm, p1, kf1["raw_xy"][idx1], d1)
        X2 = unproject_stereo(prm, p2, kf2["raw_xy"][idx2], d2)
    st1 = ~tri & s1 & (cos1 < cos2)
    st2 = ~tri & ~st1 & s2 & (cos2 < cos1)
    status = np.full(N, LOW_PARALLAX, np.int64)
    status[tri] = np.where(x4[tri, 3] == 0, W_ZERO, TRIANGULATED)
    status[st1] = np.where(d1[st1] > 0, STEREO1, LOW_PARALLAX)
    status[st2] = np.where(d2[st2] > 0, STEREO2, LOW_PARALLAX)
    X = np.where((status == TRIANGULATED)[:, None], Xt, np.where((status == STEREO1)[:, None], X1, np.where((status == STEREO2)[:, None], X2, F32(0)))).astype(F32)
    made = np.isin(status, CREATED)
    with np.errstate(all="ignore"):
        z1 = (dot(p1["Rcw"][2], X) + F64(p1["tcw"][2])).astype(F32)
        z2 = (dot(p2["Rcw"][2], X) + F64(p2["tcw"][2])).astype(F32)
        bad1, e1, th1 = _reproj_bad(prm, p1, X, z1, kp1, ur1, s1, margins, "reproj1")
        bad2, e2, th2 = _reproj_bad(prm, p2, X, z2, kp2, ur2, s2, margins, "reproj2")
        n1v, n2v = X - p1["Ow"][None], X - p2["Ow"][None]
        nd1, nd2 = norm(n1v), norm(n2v)
        dist1, dist2 = nd1.astype(F32), nd2.astype(F32)
        ratio_dist = dist2 / dist1
        ratio_factor = F32(1.5) * prm["scale_factor"]
        o1 = np.clip(kp1["octave"], 0, prm["nlevels"] - 1); o2 = np.clip(kp2["octave"], 0, prm["nlevels"] - 1)
        ratio_oct = prm["scale_factors"][o1] / prm["scale_factors"][o2]
        bad_scale = (ratio_dist * ratio_factor < ratio_oct) | (ratio_dist > ratio_oct * ratio_factor)
        acc = F32(0.0) + (n2v.astype(F64) * (F64(1.0) / nd2)[:, None]).astype(F32)
        acc = acc + (n1v.astype(F64) * (F64(1.0) / nd1)[:, None]).astype(F32)
        normal = (acc.astype(F64) * 0.5).astype(F32)
        dmax = dist1 * prm["scale_factors"][o1]
        dmin = dmax / prm["scale_factors"][prm["nlevels"] - 1]
    final = status.copy()
    alive = made.copy()
    for cond, code in ((z1 <= 0, Z1), (z2 <= 0, Z2), (bad1, REPROJ1), (bad2, REPROJ2), ((dist1 == 0) | (dist2 == 0), ZERO_DIST), (bad_scale, SCALE)):
        hit = alive & cond
        final[hit] = code
        alive &= ~cond
    if margins is not None:
        for k in range(N):
            # cosines are compared through 1 - cos, the quantity that carries their precision near 1
            sc = lambda a, b: max(abs(1.0 - float(a)), abs(1.0 - float(b)))
            margins.append(("cos_rays<cos_stereo", float(cos_rays[k]), float(cos_st[k]), sc(cos_rays[k], cos_st[k])))
            margins.append(("cos_rays>0", float(cos_rays[k]), 0.0, 1.0))
            if not (s1[k] or s2[k]):
                margins.append(("cos_rays<0.9998", float(cos_rays[k]), 0.9998, sc(cos_rays[k], 0.9998)))
            if not tri[k] and (s1[k] or s2[k]):
                margins.append(("cos1<cos2", float(cos1[k]), float(cos2[k]), sc(cos1[k], cos2[k])))
            if not made[k]:
                continue
            scale = float(max(dist1[k], dist2[k]))
            margins.append(("z1", float(z1[k]), 0.0, scale))
            if final[k] == Z1:
                continue
            margins.append(("z2", float(z2[k]), 0.0, scale))
            if final[k] == Z2:
                continue
            margins.append(("reproj1", float(e1[k]), float(th1[k]), float(th1[k])))
            if final[k] == REPROJ1:
                continue
            margins.append(("reproj2", float(e2[k]), float(th2[k]), float(th2[k])))
            if final[k] in (REPROJ2, ZERO_DIST):
                continue
            margins.append(("scale_lo", float(ratio_dist[k] * ratio_factor), float(ratio_oct[k]), float(ratio_oct[k])))
            margins.append(("scale_hi", float(ratio_dist[k]), float(ratio_oct[k] * ratio_factor), float(ratio_oct[k] * ratio_factor)))
    ok = np.isin(final, CREATED)
    out["status"] = final
    out["xyz"] = np.where(ok[:, None], X, F32(0)).astype(F32)
    out["normal"] = np.where(ok[:, None], normal, F32(0)).astype(F32)
    out["dist"] = np.where(ok[:, None], np.stack([dmin, dmax], -1), F32(0)).astype(F32)
    out["cos"] = np.stack([cos_rays, cos1, cos2], -1).astype(F32)
    out["x3d"] = np.where(tri[:, None], x4, F32(0)).astype(F32)
    out["X_all"] = X
    out["A"] = A
    out["tri"] = tri
    return out


# ---- CreateNewMapPoints ---------------------------------------------------------------------------------------------------------------------
def create_new_map_points(prm, table, cur, neighbours, use_mask=True, margins=None):
    """One item: KF1 = table[cur] against table[k] for k in neighbours, in order.  Returns per neighbour match12 / status (n1,) and nmatches,
    per idx1 the created point, new_order, and a trace (geometry, candidates before the cull, ties, epipole rejections) per neighbour.
    use_mask = False is the wrong function that forgets AddMapPoint(pMP, idx1) between neighbours (for the tests of the scenes)."""
    kf1 = table[cur]
    n1 = len(kf1["kps_un"])
    held1 = np.asarray(kf1["held"]) != 0
    R = len(neighbours)
    out = dict(match12=np.full((R, n1), -1, np.int32), status=np.zeros((R, n1), np.uint8), nmatches=np.zeros(R, np.int32),
               new_neigh=np.full(n1, -1, np.int32), new_idx2=np.full(n1, -1, np.int32), new_xyz=np.zeros((n1, 3), F32), new_normal=np.zeros((n1, 3), F32),
               new_dist=np.zeros((n1, 2), F32), new_desc=np.zeros((n1, 32), np.uint8), new_order=[], trace=[])
    for r, k2 in enumerate(neighbours):
        kf2 = table[k2]
        geo = pair_geometry(prm, kf1["Tcw"], kf2["Tcw"], margins)
        tr = dict(geo=geo, ties=[], epipole_rejects=[], skipped=geo["skip"])
        out["trace"].append(tr)
        if geo["skip"]:
            out["status"][r, :] = NEIGHBOUR_SKIPPED
            continue
        match, nm, info = search_for_triangulation(prm, kf1, kf2, geo, held1, tr, margins)
        tr.update(info)
        out["match12"][r] = match
        out["nmatches"][r] = nm
        i1 = np.nonzero(match >= 0)[0]                                  # vMatchedPairs: ascending idx1
        v = verdicts(prm, kf1, kf2, geo, i1, match[i1], margins)
        tr["verdict"] = dict(idx1=i1, **v)
        b1 = np.nonzero(info["before"] >= 0)[0]                         # every candidate before the cull (the debug accessor's view)
        tr["cand"] = dict(idx1=b1, idx2=info["before"][b1], **verdicts(prm, kf1, kf2, geo, b1, info["before"][b1]))
        for q, idx1 in enumerate(i1):
            out["status"][r, idx1] = v["status"][q]
            if v["status"][q] in CREATED:
                idx2 = int(match[idx1])
                out["new_neigh"][idx1] = r; out["new_idx2"][idx1] = idx2
                out["new_xyz"][idx1] = v["xyz"][q]; out["new_normal"][idx1] = v["normal"][q]; out["new_dist"][idx1] = v["dist"][q]
                out["new_desc"][idx1] = kf2["desc"][idx2]               # two observations: the first in creation order, the older KF2
                out["new_order"].append(int(idx1))
                if use_mask:
                    held1 = held1.copy(); held1[idx1] = True            # mpCurrentKeyFrame->AddMapPoint(pMP, idx1)
    out["new_order"] = np.array(out["new_order"], np.int32)
    return out

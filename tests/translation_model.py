"""Sequential CPU model of Optimizer::TranslationOptimization (reference src/Optimizer.cc:592-1009), the optimiser of Manhattan-mode
tracking (Tracking::TranslationWithMotionModel, src/Tracking.cc:946-1050), in IEEE double.  It is the parity reference of
msl_pose_optimize_translation[_batch] (tests/test_translation_gpu.py), as tests/pose_model.py is for PoseOptimization.

The solver is PoseOptimization's (one VertexSE3Expmap, BlockSolver_6_3, LinearSolverDense, Levenberg-Marquardt), so this file reuses
tests/pose_model.py's g2o / Eigen restatement (SE3Quat, Plane3D, LDLT, optimize, robustify) and only restates what differs: the edges
(g2o types in Thirdparty/g2o/g2o/types/types_six_dof_expmap.{h,cpp}), the counting, the early return and the classification.
pose_model.optimize evaluates edges through that module's compute_error / jacobian; translation_edges() points those two names at the
*OnlyTranslation versions below for the duration of a call.

A frame is a pose_model frame dict.  Only plane_coef, plane_w, plane_has and plane_outlier of the plane entries are read (the reference
creates no parallel or vertical plane edges here); par_outlier / ver_outlier come back unchanged.  rcw: None or manhattanRcw as 9
row-major floats, written into Tcw's rotation block first (src/Tracking.cc:974).
"""
import contextlib
import math

import numpy as np

from tests import pose_model as pm
from tests.local_match_model import gemm3

MONO, STEREO, LINE, PLANE = pm.MONO, pm.STEREO, pm.LINE, pm.PLANE


def effective_tcw(Tcw, rcw):
    """Rows 0-2 of mTcw after manhattanRcw.copyTo(mTcw.rowRange(0,3).colRange(0,3)) (src/Tracking.cc:974): a float copy."""
    T = np.array(Tcw, np.float32, copy=True).reshape(3, 4)
    if rcw is not None:
        T[:, :3] = np.asarray(rcw, np.float32).reshape(3, 3)
    return T.reshape(12)


def map_trans(T, X):                                                          # SE3Quat::mapTrans: xyz + _t
    return (X[0] + T[1][0], X[1] + T[1][1], X[2] + T[1][2])


def plane_add(T, Xc):
    """plane_3d.h:136-145 operator+(Isometry3D, Plane3D): the translation only; negated when d < 0, then Plane3D(v) normalises."""
    t = T[1]
    v = (Xc[0], Xc[1], Xc[2], Xc[3] - (t[0] * Xc[0] + t[1] * Xc[1] + t[2] * Xc[2]))
    if v[3] < 0.0:
        v = tuple(-x for x in v)
    return pm.plane_normalize(v)


def compute_error(e, T, c):
    """computeError of EdgeSE3ProjectXYZOnlyTranslation, EdgeStereoSE3ProjectXYZOnlyTranslation, EdgeLineProjectXYZOnlyTranslation
    (project(mapTrans(Xc))) and EdgePlaneOnlyTranslation ((w2n + Xc).ominus(measurement))."""
    k = e.kind
    if k == PLANE:
        return pm.ominus(plane_add(T, e.X), e.obs)
    p = map_trans(T, e.X)
    if k == STEREO:                                                           # types_six_dof_expmap.cpp:203-211: const float invz
        invz = pm.f32(1.0 / p[2])
        u = p[0] * invz * c["fx"] + c["cx"]
        return (e.obs[0] - u, e.obs[1] - (p[1] * invz * c["fy"] + c["cy"]), e.obs[2] - (u - c["bf"] * invz))
    u = p[0] / p[2] * c["fx"] + c["cx"]
    v = p[1] / p[2] * c["fy"] + c["cy"]
    if k == MONO:
        return (e.obs[0] - u, e.obs[1] - v)
    return (e.obs[0] * u + e.obs[1] * v + e.obs[2], 0.0, 0.0)


def jacobian(e, T, c):
    """linearizeOplus of the *OnlyTranslation edges: columns 0-2 (rotation) are zero.  Points and lines: the analytic translation
    columns (types_six_dof_expmap.cpp:239-268, :297-319; .h EdgeLineProjectXYZOnlyTranslation).  Planes: BaseUnaryEdge's central
    differences through oplus (base_unary_edge.hpp:82-123), then columns 0-2 zeroed (EdgePlaneOnlyTranslation::linearizeOplus)."""
    if e.kind == PLANE:
        scalar = 1.0 / (2 * pm.NUM_DELTA)
        J = [[0.0] * 6 for _ in range(3)]
        for d in range(3, 6):
            u = [0.0] * 6
            u[d] = pm.NUM_DELTA
            e1 = compute_error(e, pm.oplus(T, u), c)
            u[d] = -pm.NUM_DELTA
            e2 = compute_error(e, pm.oplus(T, u), c)
            for i in range(3):
                J[i][d] = scalar * (e1[i] - e2[i])
        return J
    x, y, z = map_trans(T, e.X)
    invz = 1.0 / z
    invz_2 = invz * invz
    fx, fy = c["fx"], c["fy"]
    if e.kind == LINE:
        lx, ly = e.obs[0], e.obs[1]
        return [[0.0, 0.0, 0.0, fx * lx * invz, fy * ly * invz, -(fx * lx * x + fy * ly * y) * invz_2], [0.0] * 6, [0.0] * 6]
    J = [[0.0, 0.0, 0.0, -invz * fx, 0.0, x * invz_2 * fx],
         [0.0, 0.0, 0.0, 0.0, -invz * fy, y * invz_2 * fy]]
    if e.kind == STEREO:
        J.append([0.0, 0.0, 0.0, J[0][3], 0.0, J[0][5] - c["bf"] * invz_2])
    return J


@contextlib.contextmanager
def translation_edges():
    """pose_model.optimize / build_system with the *OnlyTranslation error and Jacobian."""
    saved = pm.compute_error, pm.jacobian
    pm.compute_error, pm.jacobian = compute_error, jacobian
    try:
        yield
    finally:
        pm.compute_error, pm.jacobian = saved


def rotate(Tf, X):
    """cv::Mat Xc = R_cw * Xw with R_cw = mTcw(0:3, 0:3) and Xw CV_32F: cv::gemm's float kernel, as double (Optimizer.cc:616, :663, :703)."""
    return tuple(float(v) for v in gemm3(np.asarray(Tf, np.float32).reshape(3, 4), False, 1.0, np.asarray(X, np.float32)))


def build_edges(fr, c, Tf, xcap=None):
    """Optimizer.cc:635-793: point edges by keypoint index (mono when mvuRight < 0), then per line its start and end edges.  Only points
    count in nInitialCorrespondences.  Point references and octaves as pose_model.point_ref reads them.  Returns (edges, nInitial)."""
    edges = []
    n0 = 0
    for i in range(len(fr["pt_ref"])):
        ref = pm.point_ref(fr, c, i, xcap)
        if ref is None:
            continue
        r, inv = ref
        n0 += 1
        X = rotate(Tf, fr["xyz"][r])
        u, v = float(fr["un_xy"][i][0]), float(fr["un_xy"][i][1])
        if fr["uright"][i] < 0:
            edges.append(pm.Edge(MONO, i, (u, v), X, (inv, inv), pm.DELTA_MONO))
        else:
            edges.append(pm.Edge(STEREO, i, (u, v, float(fr["uright"][i])), X, (inv, inv, inv), pm.DELTA_STEREO))
    for i in range(len(fr["line_has"])):
        if not fr["line_has"][i]:
            continue
        obs = tuple(float(v) for v in fr["line_fn"][i])
        L = np.asarray(fr["line_xyz"][i], np.float64)
        for X in (L[:3], L[3:]):                                              # :755-756, :781-782: R_cw * Converter::toCvVec(...) (float)
            edges.append(pm.Edge(LINE, i, obs, rotate(Tf, X.astype(np.float32)), (1.0, 1.0, 1.0), pm.DELTA_STEREO))
    return edges, n0


def build_plane_edges(fr, c, Tf):
    """Optimizer.cc:817-861, only past the early return: one EdgePlaneOnlyTranslation per mvpMapPlanes entry.  The world plane is flipped
    against the vertex's initial pose (its rotation through the quaternion) and aTh, then Pw3D.rotateNormal(toMatrix3d(R_cw)), which
    does not renormalise."""
    Rinit = pm.quat_to_matrix(pm.to_se3(Tf)[0])
    Rd = [[float(Tf[4 * i + j]) for j in range(3)] for i in range(3)]
    info, delta = (c["angleInfo"], c["angleInfo"], c["disInfo"]), math.sqrt(c["planeChi"])
    edges = []
    for i in range(len(fr["plane_has"])):
        if not fr["plane_has"][i]:
            continue
        meas = pm.to_plane3d(fr["plane_coef"][i])
        Pw = pm.to_plane3d(fr["plane_w"][i])
        n = pm.matvec(Rinit, Pw[:3])
        pc = [float(v) for v in fr["plane_coef"][i]]
        if n[0] * pc[0] + n[1] * pc[1] + n[2] * pc[2] < -c["aTh"]:
            Pw = pm.plane_normalize(tuple(-v for v in Pw))                     # Pw3D.fromVector(-Pw)
        nr = pm.matvec(Rd, Pw[:3])
        edges.append(pm.Edge(PLANE, i, meas, (nr[0], nr[1], nr[2], Pw[3]), info, delta))
    return edges


def classify(edges, out, T, c, rows=None):
    """The classification after one round (Optimizer.cc:886-996) at the estimate T: an edge flagged last round (its out byte set) is
    re-evaluated at T, an active one is judged on the error the last trial left in it.  Line endpoints follow the same rule (:943;
    PoseOptimization re-evaluates lines always) and bad lines are not counted (nLineBad is never used); bad planes are.  Updates out and
    the edge levels; returns nBad."""
    line_th = pm.f32(2 * pm.CHI2_MONO)                                        # 2 * chi2Mono[it] in float
    nbad = 0
    lines = {}
    if rows is not None:
        rows.clear()
    for e in edges:
        key = pm.OUT_KEYS[e.kind]
        if e.kind == LINE:
            lines.setdefault(e.idx, []).append(e)
            if len(lines[e.idx]) < 2:
                continue
            e1, e2 = lines[e.idx]
            if out[key][e.idx]:
                e1.err = compute_error(e1, T, c)
                e2.err = compute_error(e2, T, c)
            a, b = pm.f32(e1.err[0] * e1.err[0]), pm.f32(e2.err[0] * e2.err[0])   # chiline() as float
            if rows is not None:
                rows += [(LINE, e.idx, a, line_th), (LINE, e.idx, b, line_th)]
            bad = a > line_th or b > line_th
            out[key][e.idx] = 1 if bad else 0
            e1.level = e2.level = 1 if bad else 0
            continue
        if out[key][e.idx]:
            e.err = compute_error(e, T, c)
        x2 = pm.f32(pm.chi2(e))
        th = {MONO: pm.CHI2_MONO, STEREO: pm.CHI2_STEREO, PLANE: c["planeChi"]}[e.kind]
        if rows is not None:
            rows.append((e.kind, e.idx, x2, th))
        if x2 > th:                                                           # bad planes count in nBad too (:985-988)
            out[key][e.idx] = 1
            e.level = 1
            nbad += 1
        else:
            out[key][e.idx] = 0
            e.level = 0
    return nbad


def translation_optimization(fr, c, rcw=None, rows=None, xcap=None):
    """int Optimizer::TranslationOptimization(Frame*) for one frame; c as for pose_model.pose_optimization.  Returns (n_good, Tcw_out (12,)
    f32, outlier arrays dict).  rows (a list, optional) receives every comparison of the last classification as (kind, index, chi2 as
    compared, threshold), for the margin check of tests/translation_scenes.py.  xcap as for pose_model.pose_optimization."""
    out = {k: np.array(fr[k], np.uint8, copy=True) for k in set(pm.OUT_KEYS.values())}
    Tf = effective_tcw(fr["Tcw"], rcw)
    edges, n0 = build_edges(fr, c, Tf, xcap)
    for e in edges:                                                           # mvbOutlier / mvbLineOutlier = false
        out[pm.OUT_KEYS[e.kind]][e.idx] = 0
    if n0 < 3:                                                                # :796, before any plane edge: plane flags untouched
        return 0, Tf, out
    planes = build_plane_edges(fr, c, Tf)
    for e in planes:
        out["plane_outlier"][e.idx] = 0
    edges += planes
    T0 = pm.to_se3(Tf)
    nbad = 0
    T = T0
    with translation_edges():
        for it in range(4):
            T = pm.optimize(edges, T0, c, 10)                                 # the estimate restarts from mTcw every round (:882)
            nbad = classify(edges, out, T, c, rows)
            if it == 2:
                for e in edges:
                    e.robust = False
            if len(edges) < 10:                                               # :998
                break
    return n0 - nbad, pm.to_cv(T), out

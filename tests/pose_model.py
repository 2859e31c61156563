"""Sequential CPU model of Optimizer::PoseOptimization (reference src/Optimizer.cc:53-590) with the vendored g2o it runs on, in IEEE
double, restated step by step (Eigen is not available, so nothing here is compiled from the reference).  It is the parity reference of
msl_pose_optimize[_batch] (tests/test_pose_gpu.py), as tests/local_match_model.py is for the local-map search.

Paths are relative to the reference repository; g2o paths to Thirdparty/g2o/g2o/.  Where Eigen's operation order is not fixed by the
source (SIMD reductions, LDLT's inner products) the sequential order is taken and the kernel (manhattanslam_amd/csrc/msl_pose.hip) does the
same per edge; DESIGN.md section 3 lists those unpinned choices.

A frame is a dict of numpy arrays (the msl_pose_optimize inputs of one frame, see pose_optimization):
  octave (N,) i32, un_xy (N,2) f32, uright (N,) f32, pt_ref (N,) i32 (-1 = no MapPoint), xyz (X,3) f32, outlier (N,) u8
  line_fn (NL,3) f64, line_xyz (NL,6) f64, line_has (NL,) u8, line_outlier (NL,) u8
  plane_coef (M,4) f32, plane_w / par_w / ver_w (M,4) f32, plane_has / par_has / ver_has (M,) u8,
  plane_outlier / par_outlier / ver_outlier (M,) u8
  Tcw (12,) f32: rows 0-2 of the CV_32F mTcw
"""
import math
import sys

import numpy as np

DBL_MAX = sys.float_info.max
CHI2_MONO = float(np.float32(5.991))                                  # Optimizer.cc:401-402 (const float arrays)
CHI2_STEREO = float(np.float32(7.815))
DELTA_MONO = float(np.float32(math.sqrt(5.991)))                     # :88-89: const float deltaMono = sqrt(5.991)
DELTA_STEREO = float(np.float32(math.sqrt(7.815)))
TAU, LOWER, UPPER, MAX_TRIALS = 1e-5, 1. / 3., 2. / 3., 10           # optimization_algorithm_levenberg.cpp:42-51
NUM_DELTA = 1e-9                                                      # base_unary_edge.hpp:95


def f32(x):
    return float(np.float32(x))


# ---- Eigen quaternion / matrix operations (coefficients (x, y, z, w) as Eigen stores them) ----

def cross(a, b):                                                      # Eigen/src/Geometry/OrthoMethods.h: cross
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def matvec(R, v):
    return tuple(R[i][0] * v[0] + R[i][1] * v[1] + R[i][2] * v[2] for i in range(3))


def matTvec(R, v):                                                    # R.transpose() * v
    return tuple(R[0][i] * v[0] + R[1][i] * v[1] + R[2][i] * v[2] for i in range(3))


def matmul(A, B):
    return [[A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def quat_normalize(q):                                                # QuaternionBase::normalize: coeffs /= sqrt(squaredNorm) if > 0
    n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    if n2 > 0:
        n = math.sqrt(n2)
        return (q[0] / n, q[1] / n, q[2] / n, q[3] / n)
    return q


def normalize_rotation(q):                                            # se3quat.h: normalizeRotation
    if q[3] < 0:
        q = (-q[0], -q[1], -q[2], -q[3])
    return quat_normalize(q)


def quat_from_matrix(m):                                              # Eigen quaternionbase_assign_impl<Matrix3>
    t = m[0][0] + m[1][1] + m[2][2]
    if t > 0:
        t = math.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        return ((m[2][1] - m[1][2]) * t, (m[0][2] - m[2][0]) * t, (m[1][0] - m[0][1]) * t, w)
    i = 0
    if m[1][1] > m[0][0]:
        i = 1
    if m[2][2] > m[i][i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    t = math.sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0)
    c = [0.0, 0.0, 0.0, 0.0]
    c[i] = 0.5 * t
    t = 0.5 / t
    c[3] = (m[k][j] - m[j][k]) * t
    c[j] = (m[j][i] + m[i][j]) * t
    c[k] = (m[k][i] + m[i][k]) * t
    return tuple(c)


def quat_to_matrix(q):                                                # QuaternionBase::toRotationMatrix
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[1 - (tyy + tzz), txy - twz, txz + twy],
            [txy + twz, 1 - (txx + tzz), tyz - twx],
            [txz - twy, tyz + twx, 1 - (txx + tyy)]]


def quat_mul(a, b):                                                   # Eigen quat_product (generic)
    return (a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
            a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
            a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
            a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2])


def quat_rotate(q, v):                                                # QuaternionBase::_transformVector
    uv = cross(q[:3], v)
    uv = (uv[0] + uv[0], uv[1] + uv[1], uv[2] + uv[2])
    c = cross(q[:3], uv)
    return tuple(v[i] + q[3] * uv[i] + c[i] for i in range(3))


# ---- SE3Quat (types/se3quat.h) ----

def se3_from_Rt(R, t):                                                # SE3Quat(Matrix3d, Vector3d): Quaterniond(R), normalizeRotation
    return (normalize_rotation(quat_from_matrix(R)), tuple(t))


def se3_mul(a, b):                                                    # se3quat.h operator*
    qa, ta = a
    qb, tb = b
    r = quat_rotate(qa, tb)
    return (normalize_rotation(quat_mul(qa, qb)), (ta[0] + r[0], ta[1] + r[1], ta[2] + r[2]))


def se3_map(T, p):                                                    # SE3Quat::map: _r * xyz + _t
    r = quat_rotate(T[0], p)
    return (r[0] + T[1][0], r[1] + T[1][1], r[2] + T[1][2])


def skew(v):
    return [[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]]


def se3_exp(u):                                                       # SE3Quat::exp
    omega, upsilon = u[:3], u[3:]
    theta = math.sqrt(omega[0] * omega[0] + omega[1] * omega[1] + omega[2] * omega[2])
    Om = skew(omega)
    Om2 = matmul(Om, Om)
    I = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    if theta < 0.00001:
        R = [[I[i][j] + Om[i][j] + Om2[i][j] for j in range(3)] for i in range(3)]
        V = R
    else:
        a, b = math.sin(theta) / theta, (1 - math.cos(theta)) / (theta * theta)
        c = (theta - math.sin(theta)) / math.pow(theta, 3)
        R = [[I[i][j] + a * Om[i][j] + b * Om2[i][j] for j in range(3)] for i in range(3)]
        V = [[I[i][j] + b * Om[i][j] + c * Om2[i][j] for j in range(3)] for i in range(3)]
    return (normalize_rotation(quat_from_matrix(R)), matvec(V, upsilon))


def se3_inverse(T):
    q = (-T[0][0], -T[0][1], -T[0][2], T[0][3])
    r = quat_rotate(q, (-T[1][0], -T[1][1], -T[1][2]))
    return (q, r)


def oplus(T, u):                                                      # VertexSE3Expmap::oplusImpl: exp(update) * estimate
    return se3_mul(se3_exp(u), T)


def to_se3(Tcw):                                                      # Converter::toSE3Quat (src/Converter.cc:35-44), float -> double
    T = [float(x) for x in Tcw]
    return se3_from_Rt([T[0:3], T[4:7], T[8:11]], (T[3], T[7], T[11]))


def to_cv(T):                                                         # to_homogeneous_matrix + Converter::toCvMat: float cast
    R = quat_to_matrix(T[0])
    return np.array([R[0][0], R[0][1], R[0][2], T[1][0], R[1][0], R[1][1], R[1][2], T[1][1], R[2][0], R[2][1], R[2][2], T[1][2]],
                    np.float32)


# ---- Plane3D (types/plane_3d.h) ----

def plane_normalize(c):                                               # Plane3D::normalize
    n = math.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])
    s = 1. / n
    c = tuple(x * s for x in c)
    if c[3] < 0.0:
        c = tuple(-x for x in c)
    return c


def to_plane3d(coe):                                                  # Converter::toPlane3D (src/Converter.cc:102-111)
    V = tuple(float(x) for x in coe)
    if float(coe[3]) < 0.0:
        V = tuple(-x for x in V)
    return plane_normalize(V)


def azimuth(v):
    return math.atan2(v[1], v[0])


def elevation(v):
    return math.atan2(v[2], math.sqrt(v[0] * v[0] + v[1] * v[1]))


def plane_rotation(v):                                                # Plane3D::rotation: (AngleAxis(az, Z) * AngleAxis(-el, Y)).toRotationMatrix()
    az, el = azimuth(v), elevation(v)
    ha, hb = 0.5 * az, 0.5 * -el
    sa, sb = math.sin(ha), math.sin(hb)
    qa = (sa * 0.0, sa * 0.0, sa * 1.0, math.cos(ha))
    qb = (sb * 0.0, sb * 1.0, sb * 0.0, math.cos(hb))
    return quat_to_matrix(quat_mul(qa, qb))


def angle_axis_matrix(angle, axis):                                   # Eigen AngleAxis::toRotationMatrix
    s, c = math.sin(angle), math.cos(angle)
    sa = tuple(s * a for a in axis)
    ca = tuple((1 - c) * a for a in axis)
    R = [[0.0] * 3 for _ in range(3)]
    tmp = ca[0] * axis[1]
    R[0][1], R[1][0] = tmp - sa[2], tmp + sa[2]
    tmp = ca[0] * axis[2]
    R[0][2], R[2][0] = tmp + sa[1], tmp - sa[1]
    tmp = ca[1] * axis[2]
    R[1][2], R[2][1] = tmp - sa[0], tmp + sa[0]
    for i in range(3):
        R[i][i] = ca[i] * axis[i] + c
    return R


def plane_transform(T, P):                                            # plane_3d.h operator*(Isometry3D, Plane3D)
    R = quat_to_matrix(T[0])
    n = matvec(R, P[:3])
    t = T[1]
    d = P[3] - (t[0] * n[0] + t[1] * n[1] + t[2] * n[2])
    v = (n[0], n[1], n[2], d)
    if v[3] < 0.0:
        v = tuple(-x for x in v)
    return plane_normalize(v)


def ominus(P, M):                                                     # Plane3D::ominus
    n = matTvec(plane_rotation(P[:3]), M[:3])
    return (azimuth(n), elevation(n), -P[3] - -M[3])


def ominus_par(P, M):                                                 # Plane3D::ominus_par
    nor = P[:3]
    if M[0] * nor[0] + M[1] * nor[1] + M[2] * nor[2] < 0:
        nor = (-nor[0], -nor[1], -nor[2])
    n = matTvec(plane_rotation(nor), M[:3])
    return (azimuth(n), elevation(n))


def ominus_ver(P, M):                                                 # Plane3D::ominus_ver
    v = cross(P[:3], M[:3])
    vn = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    b = matvec(angle_axis_matrix(math.pi / 2, (v[0] / vn, v[1] / vn, v[2] / vn)), P[:3])
    n = matTvec(plane_rotation(b), M[:3])
    return (azimuth(n), elevation(n))


# ---- edges (types/types_six_dof_expmap.{h,cpp}) ----
MONO, STEREO, LINE, PLANE, PAR, VER = range(6)


class Edge:
    __slots__ = ("kind", "idx", "obs", "X", "info", "delta", "robust", "level", "err")

    def __init__(self, kind, idx, obs, X, info, delta):
        self.kind, self.idx, self.obs, self.X, self.info, self.delta = kind, idx, obs, X, info, delta
        self.robust, self.level, self.err = True, 0, None


def compute_error(e, T, c):
    k = e.kind
    if k <= LINE:
        p = se3_map(T, e.X)
        if k == STEREO:                                                   # cam_project: const float invz = 1.0f / trans_xyz[2]
            invz = f32(1.0 / p[2])
            u = p[0] * invz * c["fx"] + c["cx"]
            return (e.obs[0] - u, e.obs[1] - (p[1] * invz * c["fy"] + c["cy"]), e.obs[2] - (u - c["bf"] * invz))
        u = p[0] / p[2] * c["fx"] + c["cx"]                                # project2d / g2o::project, then * f + c
        v = p[1] / p[2] * c["fy"] + c["cy"]
        if k == MONO:
            return (e.obs[0] - u, e.obs[1] - v)
        return (e.obs[0] * u + e.obs[1] * v + e.obs[2], 0.0, 0.0)        # EdgeLineProjectXYZOnlyPose::computeError
    local = plane_transform(T, e.X)
    if k == PLANE:
        return ominus(local, e.obs)
    if k == PAR:
        return ominus_par(local, e.obs)
    return ominus_ver(local, e.obs)


def jacobian(e, T, c):
    k = e.kind
    if k >= PLANE:                                                        # BaseUnaryEdge::linearizeOplus: central differences through oplus
        scalar = 1.0 / (2 * NUM_DELTA)
        cols = []
        for d in range(6):
            u = [0.0] * 6
            u[d] = NUM_DELTA
            e1 = compute_error(e, oplus(T, u), c)
            u[d] = -NUM_DELTA
            e2 = compute_error(e, oplus(T, u), c)
            cols.append([scalar * (a - b) for a, b in zip(e1, e2)])
        return [[cols[d][i] for d in range(6)] for i in range(len(cols[0]))]
    x, y, z = se3_map(T, e.X)
    invz = 1.0 / z
    invz_2 = invz * invz
    fx, fy = c["fx"], c["fy"]
    if k == LINE:
        lx, ly = e.obs[0], e.obs[1]
        return [[-fy * ly - fx * lx * x * y * invz_2 - fy * ly * y * y * invz_2,
                 fx * lx + fx * lx * x * x * invz_2 + fy * ly * x * y * invz_2,
                 -fx * lx * y * invz + fy * ly * x * invz,
                 fx * lx * invz, fy * ly * invz, -(fx * lx * x + fy * ly * y) * invz_2],
                [0.0] * 6, [0.0] * 6]
    J = [[x * y * invz_2 * fx, -(1 + (x * x * invz_2)) * fx, y * invz * fx, -invz * fx, 0.0, x * invz_2 * fx],
         [(1 + y * y * invz_2) * fy, -x * y * invz_2 * fy, -x * invz * fy, 0.0, -invz * fy, y * invz_2 * fy]]
    if k == STEREO:
        bf = c["bf"]
        J.append([J[0][0] - bf * y * invz_2, J[0][1] + bf * x * invz_2, J[0][2], J[0][3], 0.0, J[0][5] - bf * invz_2])
    return J


def chi2(e):                                                              # BaseEdge::chi2: error.dot(information * error), diagonal info
    s = 0.0
    for i, v in enumerate(e.err):
        s += v * (e.info[i] * v)
    return s


def robustify(e2, delta):                                                 # RobustKernelHuber::robustify (core/robust_kernel_impl.cpp:78-91)
    dsqr = delta * delta
    if e2 <= dsqr:
        return e2, 1.0
    sqrte = math.sqrt(e2)
    return 2 * sqrte * delta - dsqr, delta / sqrte


# ---- linear algebra: LinearSolverDense (solvers/linear_solver_dense.h) = Eigen::LDLT<MatrixXd> on the lower triangle ----

def ldlt_solve(A, b):
    """Eigen 3.3 ldlt_inplace<Lower>::unblocked + LDLT::_solve_impl.  Pivot rule: at step k the remaining diagonal entry of largest
    magnitude (first one on ties) is swapped to k (symmetric permutation of the lower triangle).  Returns (is_positive, x); is_positive
    is LDLT::isPositive(): no negative pivot (a zero matrix counts as positive; its pseudo-inverse solve gives x = 0)."""
    n = len(b)
    m = [[A[i][j] if j <= i else 0.0 for j in range(n)] for i in range(n)]
    tr = list(range(n))
    sign = 0                                                              # 0 ZeroSign, 1 PositiveSemiDef, -1 NegativeSemiDef, 2 Indefinite
    for k in range(n):
        idx, big = k, abs(m[k][k])
        for i in range(k + 1, n):
            if abs(m[i][i]) > big:
                idx, big = i, abs(m[i][i])
        tr[k] = idx
        if k != idx:
            for j in range(k):
                m[k][j], m[idx][j] = m[idx][j], m[k][j]
            for i in range(idx + 1, n):
                m[i][k], m[i][idx] = m[i][idx], m[i][k]
            m[k][k], m[idx][idx] = m[idx][idx], m[k][k]
            for i in range(k + 1, idx):
                m[i][k], m[idx][i] = m[idx][i], m[i][k]
        if k > 0:
            temp = [m[j][j] * m[k][j] for j in range(k)]
            s = 0.0
            for j in range(k):
                s += m[k][j] * temp[j]
            m[k][k] -= s
            for i in range(k + 1, n):
                s = 0.0
                for j in range(k):
                    s += m[i][j] * temp[j]
                m[i][k] -= s
        akk = m[k][k]
        if k == 0 and not abs(akk) > 0:
            sign, tr = 0, list(range(n))
            m = [[0.0] * n for _ in range(n)]
            break
        if abs(akk) > 0:
            for i in range(k + 1, n):
                m[i][k] /= akk
        if sign == 1:
            sign = 2 if akk < 0 else 1
        elif sign == -1:
            sign = 2 if akk > 0 else -1
        elif sign == 0:
            sign = 1 if akk > 0 else (-1 if akk < 0 else 0)
    if sign not in (0, 1):
        return False, None
    x = list(b)
    for k in range(n):                                                    # P b
        x[k], x[tr[k]] = x[tr[k]], x[k]
    for i in range(n):                                                    # L (unit lower, column sweep)
        for s in range(i + 1, n):
            x[s] -= x[i] * m[s][i]
    tiny = sys.float_info.min
    for i in range(n):                                                    # D^+ (pseudo-inverse of the diagonal)
        x[i] = x[i] / m[i][i] if abs(m[i][i]) > tiny else 0.0
    for i in range(n - 1, -1, -1):                                        # L^T (unit upper, row dot products)
        s = 0.0
        for j in range(i + 1, n):
            s += m[j][i] * x[j]
        x[i] -= s
    for k in range(n - 1, -1, -1):                                        # P^T
        x[k], x[tr[k]] = x[tr[k]], x[k]
    return True, x


# ---- g2o driver ----

def robust_chi2(edges):                                                   # SparseOptimizer::activeRobustChi2
    s = 0.0
    for e in edges:
        c2 = chi2(e)
        s += robustify(c2, e.delta)[0] if e.robust else c2
    return s


def build_system(edges, T, c):
    """BlockSolver::buildSystem for the one vertex: per active edge in order, linearizeOplus + constructQuadraticForm
    (core/base_unary_edge.hpp:43-72).  H: lower triangle, H[k][l] (l <= k) += sum_i (J_ik * w_i) * J_il with w_i = rho' * Omega_ii;
    b[k] -= sum_i ((rho' * J_ik) * Omega_ii) * e_i."""
    H = [[0.0] * 6 for _ in range(6)]
    b = [0.0] * 6
    for e in edges:
        J = jacobian(e, T, c)
        r1 = robustify(chi2(e), e.delta)[1] if e.robust else 1.0
        D = len(e.err)
        w = [r1 * e.info[i] for i in range(D)] if e.robust else list(e.info)
        for k in range(6):
            s = 0.0
            for i in range(D):
                s += ((r1 * J[i][k]) * e.info[i] if e.robust else J[i][k] * e.info[i]) * e.err[i]
            b[k] -= s
            for l in range(k + 1):
                s = 0.0
                for i in range(D):
                    s += (J[i][k] * w[i]) * J[i][l]
                H[k][l] += s
    return H, b


def optimize(edges, T, c, iterations=10):
    """SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg::solve (core/optimization_algorithm_levenberg.cpp:
    60-180).  Returns the final estimate; every active edge's err is left as the last trial evaluated it (nothing recomputes errors at
    the end: core/sparse_optimizer.cpp:376-400, no batch statistics, not verbose)."""
    active = [e for e in edges if e.level == 0]
    if not active:                                                        # no vertex in the index mapping: optimize() returns -1
        return T
    lam, ni, nbad = 0.0, 2.0, 0
    x = [0.0] * 6
    for it in range(iterations):
        for e in active:                                                  # computeActiveErrors
            e.err = compute_error(e, T, c)
        current = robust_chi2(active)
        ini = current
        H, b = build_system(active, T, c)
        if it == 0:                                                       # computeLambdaInit
            md = 0.0
            for j in range(6):
                md = max(abs(H[j][j]), md)
            lam, ni, nbad = TAU * md, 2.0, 0
        rho, q = 0.0, 0
        while True:
            Hl = [row[:] for row in H]
            for j in range(6):                                            # setLambda
                Hl[j][j] += lam
            ok, xs = ldlt_solve(Hl, b)
            if ok:
                x = xs
            trial = oplus(T, x)
            for e in active:
                e.err = compute_error(e, trial, c)
            temp = robust_chi2(active)
            if not ok:
                temp = DBL_MAX
            rho = current - temp
            scale = 0.0
            for j in range(6):
                scale += x[j] * (lam * x[j] + b[j])
            scale += 1e-3
            rho /= scale
            if rho > 0 and math.isfinite(temp):
                alpha = 1. - math.pow(2 * rho - 1, 3)
                alpha = min(alpha, UPPER)
                lam *= max(LOWER, alpha)
                ni = 2.0
                current = temp
                T = trial
            else:
                lam *= ni
                ni *= 2
            q += 1
            if not (rho < 0 and q < MAX_TRIALS):
                break
        if q == MAX_TRIALS or rho == 0:
            break
        if (ini - current) * 1e3 < ini:                                   # stop criterion (Raul)
            nbad += 1
        else:
            nbad = 0
        if nbad >= 3:
            break
    return T


def point_ref(fr, c, i, xcap=None):
    """The map point keypoint i refers to and the weight of its octave, as msl.h states them: (row of xyz, mvInvLevelSigma2 entry) or None.
    pt_ref values outside [0, xcap) (xcap: the ABI's row count per frame, default len(xyz)) count as NULL; the octave is clamped to
    [0, nlevels), nlevels = len(c["inv_level_sigma2"])."""
    r = int(fr["pt_ref"][i])
    if r < 0 or r >= (len(fr["xyz"]) if xcap is None else xcap):
        return None
    inv = c["inv_level_sigma2"]
    return r, float(inv[min(max(int(fr["octave"][i]), 0), len(inv) - 1)])


def build_edges(fr, c, xcap=None):
    """Optimizer.cc:74-377 in insertion order: points by keypoint index (mono when mvuRight < 0, else stereo), then per line its
    start-point and end-point edges, then planes, parallel planes, vertical planes.  Point references as point_ref reads them.
    Returns (edges, nInitial)."""
    T0 = to_se3(fr["Tcw"])
    edges = []
    n0 = 0
    for i in range(len(fr["pt_ref"])):
        ref = point_ref(fr, c, i, xcap)
        if ref is None:
            continue
        r, inv = ref
        n0 += 1
        X = tuple(float(v) for v in fr["xyz"][r])
        u, v = float(fr["un_xy"][i][0]), float(fr["un_xy"][i][1])
        if fr["uright"][i] < 0:
            edges.append(Edge(MONO, i, (u, v), X, (inv, inv), DELTA_MONO))
        else:
            edges.append(Edge(STEREO, i, (u, v, float(fr["uright"][i])), X, (inv, inv, inv), DELTA_STEREO))
    for i in range(len(fr["line_has"])):
        if not fr["line_has"][i]:
            continue
        n0 += 1
        obs = tuple(float(v) for v in fr["line_fn"][i])
        L = [float(v) for v in fr["line_xyz"][i]]
        edges.append(Edge(LINE, i, obs, tuple(L[:3]), (1.0, 1.0, 1.0), DELTA_STEREO))
        edges.append(Edge(LINE, i, obs, tuple(L[3:]), (1.0, 1.0, 1.0), DELTA_STEREO))
    Rinit = quat_to_matrix(T0[0])
    for kind, key, info, delta, th in ((PLANE, "plane", (c["angleInfo"], c["angleInfo"], c["disInfo"]), math.sqrt(c["planeChi"]), c["aTh"]),
                                       (PAR, "par", (c["parInfo"], c["parInfo"]), math.sqrt(c["planeChiVP"]), c["parTh"]),
                                       (VER, "ver", (c["verInfo"], c["verInfo"]), math.sqrt(c["planeChiVP"]), None)):
        for i in range(len(fr[key + "_has"])):
            if not fr[key + "_has"][i]:
                continue
            n0 += 1
            meas = to_plane3d(fr["plane_coef"][i])
            Pw = to_plane3d(fr[key + "_w"][i])
            if th is not None:                                            # :293-306: flip the world plane against the initial pose
                n = matvec(Rinit, Pw[:3])
                pc = [float(v) for v in fr["plane_coef"][i]]
                if n[0] * pc[0] + n[1] * pc[1] + n[2] * pc[2] < -th:
                    Pw = plane_normalize(tuple(-v for v in Pw))         # Pw3D.fromVector(-Pw) normalises again
            edges.append(Edge(kind, i, meas, Pw, info, delta))
    return edges, n0


OUT_KEYS = {MONO: "outlier", STEREO: "outlier", LINE: "line_outlier", PLANE: "plane_outlier", PAR: "par_outlier", VER: "ver_outlier"}


def pose_optimization(fr, c, rows=None, xcap=None):
    """int Optimizer::PoseOptimization(Frame*) for one frame.  c: fx, fy, cx, cy, bf (float values as double), inv_level_sigma2 (floats),
    angleInfo, disInfo, parInfo, verInfo, planeChi, planeChiVP, aTh, parTh.  Returns (n_good, Tcw_out (12,) f32, outlier arrays dict).
    rows (a list, optional) receives every comparison of the last classification as (kind, index, chi2 as compared, threshold): flag
    equality between two summation orders is only well defined away from the thresholds, which the scene generator checks.
    xcap: the rows of xyz a pt_ref may name (build_edges); default len(xyz)."""
    out = {k: np.array(fr[k], np.uint8, copy=True) for k in set(OUT_KEYS.values())}
    edges, n0 = build_edges(fr, c, xcap)
    for e in edges:                                                       # mvbOutlier[i] = false for every edge created
        out[OUT_KEYS[e.kind]][e.idx] = 0
    if n0 < 3:
        return 0, np.array(fr["Tcw"], np.float32, copy=True), out
    T0 = to_se3(fr["Tcw"])
    planeChi, planeChiVP = c["planeChi"], c["planeChiVP"]
    nbad = 0
    T = T0
    for it in range(4):
        T = optimize(edges, T0, c, 10)
        nbad = 0
        lines = {}
        if rows is not None:
            rows.clear()
        for e in edges:
            key = OUT_KEYS[e.kind]
            if e.kind == LINE:                                            # both endpoints: computeError every round, chiline = e0^2
                lines.setdefault(e.idx, []).append(e)
                e.err = compute_error(e, T, c)
                if len(lines[e.idx]) == 2:
                    e1, e2 = lines[e.idx]
                    th = f32(2 * CHI2_MONO)
                    a, b = f32(e1.err[0] * e1.err[0]), f32(e2.err[0] * e2.err[0])
                    if rows is not None:
                        rows += [(LINE, e.idx, a, th), (LINE, e.idx, b, th)]
                    if a > th or b > th:
                        out[key][e.idx] = 1
                        e1.level = e2.level = 1
                        nbad += 1
                    else:
                        out[key][e.idx] = 0
                        e1.level = e2.level = 0
                continue
            if out[key][e.idx]:
                e.err = compute_error(e, T, c)
            x2 = f32(chi2(e))
            th = {MONO: CHI2_MONO, STEREO: CHI2_STEREO, PLANE: planeChi, PAR: planeChiVP, VER: planeChiVP}[e.kind]
            if rows is not None:
                rows.append((e.kind, e.idx, x2, th))
            if x2 > th:
                out[key][e.idx] = 1
                e.level = 1
                nbad += 1
            else:
                out[key][e.idx] = 0
                e.level = 0
        if it == 2:
            for e in edges:
                e.robust = False
        if len(edges) < 10:
            break
    return n0 - nbad, to_cv(T), out

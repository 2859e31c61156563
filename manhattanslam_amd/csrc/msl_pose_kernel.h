// msl_pose_kernel.h -- device code of the batched pose optimisers: k_pose<false> = Optimizer::PoseOptimization (instantiated in
// msl_pose.hip), k_pose<true> = Optimizer::TranslationOptimization (instantiated in msl_pose_translation.hip).
//
// n_frames independent calls of PoseOptimization with every edge type it creates (g2o types in Thirdparty/g2o/g2o/types/
// types_six_dof_expmap.{h,cpp}: EdgeSE3ProjectXYZOnlyPose, EdgeStereoSE3ProjectXYZOnlyPose, EdgeLineProjectXYZOnlyPose, EdgePlaneOnlyPose,
// EdgeParallelPlaneOnlyPose, EdgeVerticalPlaneOnlyPose) and the solver it builds: OptimizationAlgorithmLevenberg over a BlockSolver_6_3
// with LinearSolverDense (Eigen::LDLT), 4 rounds x optimize(10) with the outlier classification after each round.
//
// One workgroup (4 waves) per frame; the LM state machine of a frame is sequential, so the frame is the unit of parallelism across the
// batch and its edges are the unit inside the workgroup.  Per LM iteration:
//   system pass   every lane walks its edges (item = point, line, or one plane kind of one plane; item index = lane + k * 256) and
//                 accumulates, per edge in the reference's per-edge order, the robust chi2 and constructQuadraticForm's contribution
//                 (21 lower-triangle H entries, 6 of b) in double; a fixed xor-butterfly over the wave and a fixed-order sum of the four
//                 wave totals make the sums deterministic and independent of the other frames in the batch;
//   trial         lane 0 adds lambda to the diagonal, runs the 6x6 LDLT (Eigen's diagonal pivoting, in LDS), applies SE3Quat::exp(x) *
//                 estimate; all lanes evaluate the robust chi2 at the trial pose (one reduced value); lane 0 accepts or rejects, updates
//                 lambda / ni and decides whether to try again (three barriers per trial).
// The active set is the per-edge outlier byte itself (level 1 = flagged), not a compaction.  g2o leaves an active edge's error at the
// last trial it evaluated (nothing recomputes errors when optimize() returns), so the classification evaluates such an edge at that
// trial's pose, kept in LDS.  Per-edge arithmetic follows tests/pose_model.py operation for operation; only the sums over edges differ
// in order from g2o's sequential loop.  DESIGN.md section 3 lists what is pinned and what is not.
//
// k_pose<true> is Optimizer::TranslationOptimization (src/Optimizer.cc:592-1009, Manhattan mode) on the same solver: the edges are the
// *OnlyTranslation types (points and line endpoints rotated once into the camera, Xc = R_cw * Xw in float; plane edges only for
// mvpMapPlanes), whose Jacobians have zero rotation columns, so the 6x6 system carries only lambda in its rotation block and the update
// leaves the rotation to the quaternion round trip of SE3Quat::exp * estimate.  The counting, the early return and the classification
// differ as tests/translation_model.py restates them.
//
// The two instantiations live in separate translation units and take different argument records (PoseDev, PoseDevT): in one module the
// second instantiation changes the inliner's and scheduler's choices for the first, and PoseOptimization's kernel is meant to compile to
// the same code whether or not translation mode exists.
#pragma once
#include "msl_match_handle.h"
#include "msl_match_math.h"
#include "msl_plane_tables.h"                  // MAX_PCAP: the planes of a frame, as the plane chain produces them

#include <cfloat>
#include <cmath>
#include <type_traits>

namespace msl {

struct PoseDev {
    int cap, xcap, lcap, pcap;
    msl_pose_params prm;
    double deltaMono, deltaStereo, deltaPlane, deltaPlaneVP;   // Huber deltas (Optimizer.cc:88-89 as float; sqrt(planeChi), sqrt(planeChiVP))
    const msl_keypoint *kps; const float *unxy, *uright; const int32_t *ptRef, *nKps; const float *xyz;
    const double *lineFn, *lineXyz; const uint8_t *lineHas; const int32_t *nLines;
    const float *planeCoef, *planeW; const uint8_t *planeHas; const int32_t *nPlanes;
    const float *Tcw;
    uint8_t *outlier, *lineOutlier, *planeOutlier;   // in/out
    float *TcwOut; int32_t *nGood;
};
struct PoseDevT : PoseDev {
    const float *Rcw;                                  // the Manhattan rotation (9 floats per frame, row-major) or NULL
};

// Launches k_pose<true> (msl_pose_translation.hip): one workgroup per frame on `st`.
hipError_t launch_pose_translation(const PoseDevT &D, int n_frames, hipStream_t st);

}  // namespace msl

using namespace msl;

namespace {


constexpr int MAX_XCAP = 32768;               // map points of a frame; its keylines: MAX_KLCAP (msl_match_handle.h)
constexpr int NT = 256;                       // four waves per frame
constexpr int NRED = 28;                      // 21 H (lower triangle) + 6 b + robust chi2
constexpr int MONO = 0, STEREO = 1, LINE = 2, PLANE = 3, PAR = 4, VER = 5;

struct SE3 { double q[4]; double t[3]; };   // SE3Quat: q = (x, y, z, w) as Eigen stores it

// ---- Eigen quaternion / matrix operations (same order as tests/pose_model.py) ----
__device__ inline void cross3(const double *a, const double *b, double *r) {
    r[0] = a[1] * b[2] - a[2] * b[1]; r[1] = a[2] * b[0] - a[0] * b[2]; r[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ inline void matvec(const double R[3][3], const double *v, double *r) {
    for (int i = 0; i < 3; i++) r[i] = R[i][0] * v[0] + R[i][1] * v[1] + R[i][2] * v[2];
}
__device__ inline void matTvec(const double R[3][3], const double *v, double *r) {
    for (int i = 0; i < 3; i++) r[i] = R[0][i] * v[0] + R[1][i] * v[1] + R[2][i] * v[2];
}
__device__ inline void normalize_rotation(double *q) {        // se3quat.h normalizeRotation + QuaternionBase::normalize
    if (q[3] < 0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
    const double n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    if (n2 > 0) { const double n = sqrt(n2); q[0] = q[0] / n; q[1] = q[1] / n; q[2] = q[2] / n; q[3] = q[3] / n; }
}
__device__ inline void quat_from_matrix(const double m[3][3], double *q) {   // quaternionbase_assign_impl<Matrix3>
    double t = m[0][0] + m[1][1] + m[2][2];
    if (t > 0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[2][1] - m[1][2]) * t; q[1] = (m[0][2] - m[2][0]) * t; q[2] = (m[1][0] - m[0][1]) * t;
        return;
    }
    int i = 0;
    if (m[1][1] > m[0][0]) i = 1;
    if (m[2][2] > m[i][i]) i = 2;
    const int j = (i + 1) % 3, k = (i + 2) % 3;
    t = sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0);
    q[i] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (m[k][j] - m[j][k]) * t;
    q[j] = (m[j][i] + m[i][j]) * t;
    q[k] = (m[k][i] + m[i][k]) * t;
}
__device__ inline void quat_to_matrix(const double *q, double R[3][3]) {      // QuaternionBase::toRotationMatrix
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0][0] = 1 - (tyy + tzz); R[0][1] = txy - twz; R[0][2] = txz + twy;
    R[1][0] = txy + twz; R[1][1] = 1 - (txx + tzz); R[1][2] = tyz - twx;
    R[2][0] = txz - twy; R[2][1] = tyz + twx; R[2][2] = 1 - (txx + tyy);
}
__device__ inline void quat_mul(const double *a, const double *b, double *r) { // quat_product
    r[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    r[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    r[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
    r[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}
__device__ inline void quat_rotate(const double *q, const double *v, double *r) {   // _transformVector
    double uv[3], c[3];
    cross3(q, v, uv);
    uv[0] = uv[0] + uv[0]; uv[1] = uv[1] + uv[1]; uv[2] = uv[2] + uv[2];
    cross3(q, uv, c);
    for (int i = 0; i < 3; i++) r[i] = v[i] + q[3] * uv[i] + c[i];
}
__device__ inline void se3_map(const SE3 &T, const double *p, double *r) {    // SE3Quat::map
    double a[3];
    quat_rotate(T.q, p, a);
    r[0] = a[0] + T.t[0]; r[1] = a[1] + T.t[1]; r[2] = a[2] + T.t[2];
}
__device__ inline SE3 oplus(const SE3 &T, const double *u) {                   // VertexSE3Expmap::oplusImpl: SE3Quat::exp(u) * T
    const double om[3] = {u[0], u[1], u[2]};
    const double theta = sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]);
    const double O[3][3] = {{0.0, -om[2], om[1]}, {om[2], 0.0, -om[0]}, {-om[1], om[0], 0.0}};
    double O2[3][3], R[3][3], V[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) O2[i][j] = O[i][0] * O[0][j] + O[i][1] * O[1][j] + O[i][2] * O[2][j];
    if (theta < 0.00001) {
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) { R[i][j] = (i == j ? 1.0 : 0.0) + O[i][j] + O2[i][j]; V[i][j] = R[i][j]; }
    } else {
        const double a = sin(theta) / theta, b = (1 - cos(theta)) / (theta * theta), c = (theta - sin(theta)) / pow(theta, 3.0);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                R[i][j] = (i == j ? 1.0 : 0.0) + a * O[i][j] + b * O2[i][j];
                V[i][j] = (i == j ? 1.0 : 0.0) + b * O[i][j] + c * O2[i][j];
            }
    }
    SE3 E;
    quat_from_matrix(R, E.q);
    normalize_rotation(E.q);
    matvec(V, u + 3, E.t);
    SE3 r;                                                                       // se3quat.h operator*
    double a[3];
    quat_rotate(E.q, T.t, a);
    quat_mul(E.q, T.q, r.q);
    normalize_rotation(r.q);
    r.t[0] = E.t[0] + a[0]; r.t[1] = E.t[1] + a[1]; r.t[2] = E.t[2] + a[2];
    return r;
}

// ---- Plane3D (types/plane_3d.h) ----
__device__ inline void plane_normalize(double *c) {
    const double n = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    const double s = 1. / n;
    for (int i = 0; i < 4; i++) c[i] = c[i] * s;
    if (c[3] < 0.0) for (int i = 0; i < 4; i++) c[i] = -c[i];
}
__device__ inline void to_plane3d(const float *coe, double *V) {             // Converter::toPlane3D (src/Converter.cc:102-111)
    for (int i = 0; i < 4; i++) V[i] = (double)coe[i];
    if (coe[3] < 0.0f) for (int i = 0; i < 4; i++) V[i] = -V[i];
    plane_normalize(V);
}
__device__ inline double azimuth(const double *v) { return atan2(v[1], v[0]); }
__device__ inline double elevation(const double *v) { return atan2(v[2], sqrt(v[0] * v[0] + v[1] * v[1])); }
__device__ inline void plane_rotation(const double *v, double R[3][3]) {      // (AngleAxis(az, Z) * AngleAxis(-el, Y)).toRotationMatrix()
    const double ha = 0.5 * azimuth(v), hb = 0.5 * -elevation(v);
    const double sa = sin(ha), sb = sin(hb);
    const double qa[4] = {sa * 0.0, sa * 0.0, sa * 1.0, cos(ha)}, qb[4] = {sb * 0.0, sb * 1.0, sb * 0.0, cos(hb)};
    double q[4];
    quat_mul(qa, qb, q);
    quat_to_matrix(q, R);
}
__device__ inline void plane_transform(const SE3 &T, const double *P, double *v) {   // operator*(Isometry3D, Plane3D)
    double R[3][3];
    quat_to_matrix(T.q, R);
    matvec(R, P, v);
    v[3] = P[3] - (T.t[0] * v[0] + T.t[1] * v[1] + T.t[2] * v[2]);
    if (v[3] < 0.0) for (int i = 0; i < 4; i++) v[i] = -v[i];
    plane_normalize(v);
}
// localPlane.ominus / ominus_par / ominus_ver (measurement M); returns the error dimension
__device__ inline int plane_error(int kind, const SE3 &T, const double *Pw, const double *M, double *e) {
    double P[4], R[3][3], n[3];
    plane_transform(T, Pw, P);
    if (kind == PLANE) {
        plane_rotation(P, R);
        matTvec(R, M, n);
        e[0] = azimuth(n); e[1] = elevation(n); e[2] = -P[3] - -M[3];
        return 3;
    }
    if (kind == PAR) {
        double nor[3] = {P[0], P[1], P[2]};
        if (M[0] * nor[0] + M[1] * nor[1] + M[2] * nor[2] < 0) { nor[0] = -nor[0]; nor[1] = -nor[1]; nor[2] = -nor[2]; }
        plane_rotation(nor, R);
    } else {
        double v[3], b[3], A[3][3];
        cross3(P, M, v);
        const double vn = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        const double ax[3] = {v[0] / vn, v[1] / vn, v[2] / vn};
        const double ang = M_PI / 2, s = sin(ang), c = cos(ang);                  // AngleAxis::toRotationMatrix
        const double sa[3] = {s * ax[0], s * ax[1], s * ax[2]}, ca[3] = {(1 - c) * ax[0], (1 - c) * ax[1], (1 - c) * ax[2]};
        double tmp = ca[0] * ax[1];
        A[0][1] = tmp - sa[2]; A[1][0] = tmp + sa[2];
        tmp = ca[0] * ax[2];
        A[0][2] = tmp + sa[1]; A[2][0] = tmp - sa[1];
        tmp = ca[1] * ax[2];
        A[1][2] = tmp - sa[0]; A[2][1] = tmp + sa[0];
        for (int i = 0; i < 3; i++) A[i][i] = ca[i] * ax[i] + c;
        matvec(A, P, b);
        plane_rotation(b, R);
    }
    matTvec(R, M, n);
    e[0] = azimuth(n); e[1] = elevation(n);
    return 2;
}

// ---- one edge ----
struct Edge {
    int kind, dim;
    double obs[4], X[4], info[3], delta;
};

// EdgePlaneOnlyTranslation::computeError: (w2n + Xc).ominus(measurement); operator+ (types/plane_3d.h:136-145) moves the plane by the
// translation only and negates it when d < 0
__device__ inline void plane_error_trans(const SE3 &T, const double *Xc, const double *M, double *e) {
    double v[4] = {Xc[0], Xc[1], Xc[2], 0.0}, R[3][3], n[3];
    v[3] = Xc[3] - (T.t[0] * v[0] + T.t[1] * v[1] + T.t[2] * v[2]);
    if (v[3] < 0.0) for (int i = 0; i < 4; i++) v[i] = -v[i];
    plane_normalize(v);
    plane_rotation(v, R);
    matTvec(R, M, n);
    e[0] = azimuth(n); e[1] = elevation(n); e[2] = -v[3] - -M[3];
}

__device__ inline void map_trans(const SE3 &T, const double *p, double *r) {   // SE3Quat::mapTrans: xyz + _t
    r[0] = p[0] + T.t[0]; r[1] = p[1] + T.t[1]; r[2] = p[2] + T.t[2];
}

template <bool TRANS>
__device__ inline void edge_error(const Edge &E, const SE3 &T, const PoseDev &P, double *e) {
    if (E.kind >= PLANE) {
        if constexpr (TRANS) plane_error_trans(T, E.X, E.obs, e);
        else plane_error(E.kind, T, E.X, E.obs, e);
        return;
    }
    double p[3];
    if constexpr (TRANS) map_trans(T, E.X, p);                                  // E.X is Xc
    else se3_map(T, E.X, p);
    const double fx = P.prm.fx, fy = P.prm.fy, cx = P.prm.cx, cy = P.prm.cy;
    if (E.kind == STEREO) {                                                      // cam_project: const float invz = 1.0f / trans_xyz[2]
        const double invz = (double)(float)(1.0 / p[2]);
        const double u = p[0] * invz * fx + cx;
        e[0] = E.obs[0] - u; e[1] = E.obs[1] - (p[1] * invz * fy + cy); e[2] = E.obs[2] - (u - (double)P.prm.bf * invz);
        return;
    }
    const double u = p[0] / p[2] * fx + cx, v = p[1] / p[2] * fy + cy;
    if (E.kind == MONO) { e[0] = E.obs[0] - u; e[1] = E.obs[1] - v; return; }
    e[0] = E.obs[0] * u + E.obs[1] * v + E.obs[2]; e[1] = 0.0; e[2] = 0.0;     // EdgeLineProjectXYZOnlyPose::computeError
}

__device__ inline double edge_chi2(const Edge &E, const double *e) {           // error.dot(information * error)
    double s = 0.0;
    for (int i = 0; i < E.dim; i++) s += e[i] * (E.info[i] * e[i]);
    return s;
}

__device__ inline void huber(double e2, double delta, double &rho0, double &rho1) {   // RobustKernelHuber::robustify
    const double dsqr = delta * delta;
    if (e2 <= dsqr) { rho0 = e2; rho1 = 1.; return; }
    const double sqrte = sqrt(e2);
    rho0 = 2 * sqrte * delta - dsqr; rho1 = delta / sqrte;
}

template <bool TRANS>
__device__ __noinline__ void plane_jacobian(const Edge &E, const SE3 &T, const PoseDev &P, double J[3][6]) {   // base_unary_edge.hpp:82-123
    const double delta = 1e-9, scalar = 1.0 / (2 * delta);
    for (int d = 0; d < 6; d++) {
        if constexpr (TRANS) {                                                   // EdgePlaneOnlyTranslation::linearizeOplus zeroes columns 0-2
            if (d < 3) { J[0][d] = 0.0; J[1][d] = 0.0; J[2][d] = 0.0; continue; }
        }
        double u[6] = {0, 0, 0, 0, 0, 0}, e1[3] = {0, 0, 0}, e2[3] = {0, 0, 0};
        u[d] = delta;
        edge_error<TRANS>(E, oplus(T, u), P, e1);
        u[d] = -delta;
        edge_error<TRANS>(E, oplus(T, u), P, e2);
        for (int i = 0; i < 3; i++) J[i][d] = scalar * (e1[i] - e2[i]);
    }
}

// The *OnlyTranslation Jacobians (types_six_dof_expmap.h / .cpp) are the pose ones at mapTrans(Xc) with columns 0-2 set to zero.
template <bool TRANS>
__device__ inline void edge_jacobian(const Edge &E, const SE3 &T, const PoseDev &P, double J[3][6]) {
    if (E.kind >= PLANE) { plane_jacobian<TRANS>(E, T, P, J); return; }
    double p[3];
    if constexpr (TRANS) map_trans(T, E.X, p);
    else se3_map(T, E.X, p);
    const double x = p[0], y = p[1], invz = 1.0 / p[2], invz_2 = invz * invz;
    const double fx = P.prm.fx, fy = P.prm.fy;
    if (E.kind == LINE) {
        const double lx = E.obs[0], ly = E.obs[1];
        J[0][0] = -fy * ly - fx * lx * x * y * invz_2 - fy * ly * y * y * invz_2;
        J[0][1] = fx * lx + fx * lx * x * x * invz_2 + fy * ly * x * y * invz_2;
        J[0][2] = -fx * lx * y * invz + fy * ly * x * invz;
        J[0][3] = fx * lx * invz;
        J[0][4] = fy * ly * invz;
        J[0][5] = -(fx * lx * x + fy * ly * y) * invz_2;
        for (int d = 0; d < 6; d++) { J[1][d] = 0.0; J[2][d] = 0.0; }
        if constexpr (TRANS) { J[0][0] = 0.0; J[0][1] = 0.0; J[0][2] = 0.0; }
        return;
    }
    J[0][0] = x * y * invz_2 * fx; J[0][1] = -(1 + (x * x * invz_2)) * fx; J[0][2] = y * invz * fx; J[0][3] = -invz * fx; J[0][4] = 0.0;
    J[0][5] = x * invz_2 * fx;
    J[1][0] = (1 + y * y * invz_2) * fy; J[1][1] = -x * y * invz_2 * fy; J[1][2] = -x * invz * fy; J[1][3] = 0.0; J[1][4] = -invz * fy;
    J[1][5] = y * invz_2 * fy;
    if (E.kind == STEREO) {
        const double bf = P.prm.bf;
        J[2][0] = J[0][0] - bf * y * invz_2; J[2][1] = J[0][1] + bf * x * invz_2; J[2][2] = J[0][2]; J[2][3] = J[0][3]; J[2][4] = 0.0;
        J[2][5] = J[0][5] - bf * invz_2;
    }
    if constexpr (TRANS)
        for (int i = 0; i < 3; i++) { J[i][0] = 0.0; J[i][1] = 0.0; J[i][2] = 0.0; }
}

// ---- the edges of one frame: item = point i | line j (two edges) | plane kind s of plane k (TRANS: plane k, s = 0 only) ----
template <bool TRANS>
struct Frame {
    int f, nK, nL, nP;
    const PoseDev *P;
    const float *Tf;                                                             // TRANS: rows 0-2 of mTcw with the Manhattan rotation in
    __device__ int items() const { return nK + nL + (TRANS ? nP : 3 * nP); }
    // edges of item `it` (0, 1 or 2); flag = the edge's outlier byte (level 1)
    __device__ int load(int it, Edge *E, uint8_t *&flag, const double Rinit[3][3]) const {
        const PoseDev &Q = *P;
        if (it < nK) {
            const size_t g = (size_t)f * Q.cap + it;
            const int r = Q.ptRef[g];
            if (r < 0 || r >= Q.xcap) return 0;
            const float *X = Q.xyz + ((size_t)f * Q.xcap + r) * 3;
            int oct = Q.kps[g].octave;
            oct = oct < 0 ? 0 : (oct >= Q.prm.nlevels ? Q.prm.nlevels - 1 : oct);
            const double inv = (double)Q.prm.inv_level_sigma2[oct];
            const float ur = Q.uright[g];
            E->kind = ur < 0 ? MONO : STEREO; E->dim = ur < 0 ? 2 : 3;
            E->obs[0] = Q.unxy[2 * g]; E->obs[1] = Q.unxy[2 * g + 1]; E->obs[2] = ur;
            if constexpr (TRANS) {                                               // Optimizer.cc:663-664, :703-704: cv::Mat Xc = R_cw * Xw
                float xc[3];
                gemm3(Tf, false, 1.0, X, nullptr, xc);
                E->X[0] = xc[0]; E->X[1] = xc[1]; E->X[2] = xc[2];
            } else {
                E->X[0] = X[0]; E->X[1] = X[1]; E->X[2] = X[2];
            }
            E->info[0] = inv; E->info[1] = inv; E->info[2] = inv;
            E->delta = ur < 0 ? Q.deltaMono : Q.deltaStereo;
            flag = Q.outlier + g;
            return 1;
        }
        it -= nK;
        if (it < nL) {
            const size_t g = (size_t)f * Q.lcap + it;
            if (!Q.lineHas[g]) return 0;
            for (int k = 0; k < 2; k++) {
                E[k].kind = LINE; E[k].dim = 3; E[k].delta = Q.deltaStereo;
                for (int i = 0; i < 3; i++) { E[k].obs[i] = Q.lineFn[3 * g + i]; E[k].X[i] = Q.lineXyz[6 * g + 3 * k + i]; E[k].info[i] = 1.0; }
                if constexpr (TRANS) {                                           // :755-756, :781-782: R_cw * Converter::toCvVec(mWorldPos.head / tail)
                    const float w[3] = {(float)E[k].X[0], (float)E[k].X[1], (float)E[k].X[2]};
                    float xc[3];
                    gemm3(Tf, false, 1.0, w, nullptr, xc);
                    E[k].X[0] = xc[0]; E[k].X[1] = xc[1]; E[k].X[2] = xc[2];
                }
            }
            flag = Q.lineOutlier + g;
            return 2;
        }
        it -= nL;
        const int k = TRANS ? it : it / 3, s = TRANS ? 0 : it - 3 * k;
        const size_t g = (size_t)f * Q.pcap + k;
        if (!((Q.planeHas[g] >> s) & 1)) return 0;
        const float *pc = Q.planeCoef + 4 * g;
        E->kind = PLANE + s;
        E->dim = s == 0 ? 3 : 2;
        to_plane3d(pc, E->obs);
        to_plane3d(Q.planeW + 12 * g + 4 * s, E->X);
        if (s < 2) {                                                             // Optimizer.cc:293-306 / :338-351: flip against the initial pose
            double n[3];
            matvec(Rinit, E->X, n);
            const double th = s == 0 ? Q.prm.a_th : Q.prm.par_th;
            if (n[0] * (double)pc[0] + n[1] * (double)pc[1] + n[2] * (double)pc[2] < -th) {
                for (int i = 0; i < 4; i++) E->X[i] = -E->X[i];
                plane_normalize(E->X);
            }
        }
        if constexpr (TRANS) {                                                   // :853: Pw3D.rotateNormal(toMatrix3d(R_cw)), not renormalised
            const double R[3][3] = {{Tf[0], Tf[1], Tf[2]}, {Tf[4], Tf[5], Tf[6]}, {Tf[8], Tf[9], Tf[10]}};
            double n[3];
            matvec(R, E->X, n);
            E->X[0] = n[0]; E->X[1] = n[1]; E->X[2] = n[2];
        }
        if (s == 0) { E->info[0] = Q.prm.angle_info; E->info[1] = Q.prm.angle_info; E->info[2] = Q.prm.dis_info; E->delta = Q.deltaPlane; }
        else { const double v = s == 1 ? Q.prm.par_info : Q.prm.ver_info; E->info[0] = v; E->info[1] = v; E->info[2] = 0.0; E->delta = Q.deltaPlaneVP; }
        flag = Q.planeOutlier + 3 * g + s;
        return 1;
    }
};

__device__ inline double wave_sum(double v) {                                  // xor butterfly: every lane ends with the same bits
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

struct Lm {                                                                      // lane 0's LM state, in LDS
    double H[6][6], b[6], x[6], M[6][6];
    double lambda, ni, current, ini;
    int nbad;
};

// LinearSolverDense::solve = Eigen::LDLT<MatrixXd>(H).solve(b) on the lower triangle (tests/pose_model.py ldlt_solve); returns isPositive()
__device__ bool ldlt_solve(double M[6][6], const double *b, double *x) {
    int tr[6];
    int sign = 0;                                                                // ZeroSign, 1 PositiveSemiDef, -1 NegativeSemiDef, 2 Indefinite
    bool zero = false;
    for (int k = 0; k < 6; k++) {
        int idx = k;
        double big = fabs(M[k][k]);
        for (int i = k + 1; i < 6; i++) if (fabs(M[i][i]) > big) { idx = i; big = fabs(M[i][i]); }
        tr[k] = idx;
        if (k != idx) {
            for (int j = 0; j < k; j++) { const double t = M[k][j]; M[k][j] = M[idx][j]; M[idx][j] = t; }
            for (int i = idx + 1; i < 6; i++) { const double t = M[i][k]; M[i][k] = M[i][idx]; M[i][idx] = t; }
            { const double t = M[k][k]; M[k][k] = M[idx][idx]; M[idx][idx] = t; }
            for (int i = k + 1; i < idx; i++) { const double t = M[i][k]; M[i][k] = M[idx][i]; M[idx][i] = t; }
        }
        if (k > 0) {
            double temp[6];
            for (int j = 0; j < k; j++) temp[j] = M[j][j] * M[k][j];
            double s = 0.0;
            for (int j = 0; j < k; j++) s += M[k][j] * temp[j];
            M[k][k] -= s;
            for (int i = k + 1; i < 6; i++) {
                s = 0.0;
                for (int j = 0; j < k; j++) s += M[i][j] * temp[j];
                M[i][k] -= s;
            }
        }
        const double akk = M[k][k];
        if (k == 0 && !(fabs(akk) > 0)) { zero = true; break; }
        if (fabs(akk) > 0) for (int i = k + 1; i < 6; i++) M[i][k] /= akk;
        if (sign == 1) sign = akk < 0 ? 2 : 1;
        else if (sign == -1) sign = akk > 0 ? 2 : -1;
        else if (sign == 0) sign = akk > 0 ? 1 : (akk < 0 ? -1 : 0);
    }
    if (zero) {                                                                  // all-zero diagonal: D = 0, identity permutation -> x = 0
        for (int i = 0; i < 6; i++) x[i] = 0.0;
        return true;
    }
    if (sign != 0 && sign != 1) return false;
    double v[6];
    for (int i = 0; i < 6; i++) v[i] = b[i];
    for (int k = 0; k < 6; k++) { const double t = v[k]; v[k] = v[tr[k]]; v[tr[k]] = t; }
    for (int i = 0; i < 6; i++)
        for (int s = i + 1; s < 6; s++) v[s] -= v[i] * M[s][i];
    for (int i = 0; i < 6; i++) v[i] = fabs(M[i][i]) > DBL_MIN ? v[i] / M[i][i] : 0.0;
    for (int i = 5; i >= 0; i--) {
        double s = 0.0;
        for (int j = i + 1; j < 6; j++) s += M[j][i] * v[j];
        v[i] -= s;
    }
    for (int k = 5; k >= 0; k--) { const double t = v[k]; v[k] = v[tr[k]]; v[tr[k]] = t; }
    for (int i = 0; i < 6; i++) x[i] = v[i];
    return true;
}

// Sums `n` per-lane values over the workgroup in a fixed order: the wave butterfly, then waves 0..3 in order (lane 0 reads `out`).
__device__ inline void block_sum(const double *acc, int n, double (*red)[NRED], double *out) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int k = 0; k < n; k++) {
        const double s = wave_sum(acc[k]);
        if (lane == 0) red[wv][k] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 0; k < n; k++) out[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
}

// TRANS = false: PoseOptimization; TRANS = true: TranslationOptimization (edge construction, errors, Jacobians, counting and
// classification differ; the LM machinery is shared).
template <bool TRANS>
__global__ __launch_bounds__(NT) void k_pose(std::conditional_t<TRANS, PoseDevT, PoseDev> A) {
    const PoseDev &P = A;
    const float *Rcw = nullptr;
    if constexpr (TRANS) Rcw = A.Rcw;
    __shared__ double red[4][NRED];
    __shared__ double sum[NRED];
    __shared__ SE3 sT0, sT, sTrial;
    __shared__ Lm lm;
    __shared__ double sR0[3][3];
    __shared__ int sCnt[4];                                                      // n0, edges, active, nbad
    __shared__ int sCtl[2];                                                      // another trial, stop optimize()
    __shared__ float sTf[12];                                                    // TRANS: mTcw after the Manhattan rotation is written in
    const int tid = threadIdx.x;
    Frame<TRANS> F;
    F.f = blockIdx.x; F.P = &P;
    if constexpr (TRANS) F.Tf = sTf;
    F.nK = min(max(P.nKps[F.f], 0), P.cap); F.nL = min(max(P.nLines[F.f], 0), P.lcap); F.nP = min(max(P.nPlanes[F.f], 0), P.pcap);
    const int nItems = F.items();
    if (tid == 0) {
        sCnt[0] = sCnt[1] = sCnt[2] = sCnt[3] = 0;
        const float *m = P.Tcw + 12 * (size_t)F.f;                              // Converter::toSE3Quat
        if constexpr (TRANS) {                                                   // Tracking.cc:974: manhattanRcw.copyTo(mTcw(0:3, 0:3))
            for (int i = 0; i < 12; i++) sTf[i] = m[i];
            if (Rcw)
                for (int i = 0; i < 3; i++)
                    for (int j = 0; j < 3; j++) sTf[4 * i + j] = Rcw[9 * (size_t)F.f + 3 * i + j];
            m = sTf;
        }
        const double R[3][3] = {{m[0], m[1], m[2]}, {m[4], m[5], m[6]}, {m[8], m[9], m[10]}};
        quat_from_matrix(R, sT0.q);
        normalize_rotation(sT0.q);
        sT0.t[0] = m[3]; sT0.t[1] = m[7]; sT0.t[2] = m[11];
        quat_to_matrix(sT0.q, sR0);
    }
    __syncthreads();
    Edge E[2];
    uint8_t *flag;
    // edge construction: mvbOutlier[i] = false, nInitialCorrespondences.  TranslationOptimization counts points only, and creates its
    // plane edges after the early return (Optimizer.cc:796)
    const int nBuild = TRANS ? F.nK + F.nL : nItems;
    for (int it = tid; it < nBuild; it += NT) {
        const int ne = F.load(it, E, flag, sR0);
        if (!ne) continue;
        *flag = 0;
        if (!TRANS || it < F.nK) atomicAdd(&sCnt[0], 1);
        atomicAdd(&sCnt[1], ne);
    }
    __syncthreads();
    const int n0 = sCnt[0];
    int nEdges = sCnt[1];
    if (n0 < 3) {
        if (tid < 12) P.TcwOut[12 * (size_t)F.f + tid] = TRANS ? sTf[tid] : P.Tcw[12 * (size_t)F.f + tid];
        if (tid == 0) P.nGood[F.f] = 0;
        return;
    }
    if constexpr (TRANS) {                                                       // :817-861: the plane edges, mvbPlaneOutlier[i] = false
        for (int it = nBuild + tid; it < nItems; it += NT) {
            if (!F.load(it, E, flag, sR0)) continue;
            *flag = 0;
            atomicAdd(&sCnt[1], 1);
        }
        __syncthreads();
        nEdges = sCnt[1];
    }
    int nbad = 0;
    for (int round = 0; round < 4; round++) {
        const bool robust = round < 3;
        if (tid == 0) { sT = sT0; sTrial = sT0; sCnt[2] = 0; sCnt[3] = 0; }
        __syncthreads();
        for (int it = tid; it < nItems; it += NT) {
            const int ne = F.load(it, E, flag, sR0);
            if (ne && !*flag) atomicAdd(&sCnt[2], 1);
        }
        __syncthreads();
        if (sCnt[2] > 0) {                                                       // else optimize() returns at once: no vertex to optimise
            for (int iter = 0; iter < 10; iter++) {
                // computeActiveErrors + activeRobustChi2 + buildSystem at the current estimate
                double acc[NRED];
                for (int k = 0; k < NRED; k++) acc[k] = 0.0;
                const SE3 T = sT;
                for (int it = tid; it < nItems; it += NT) {
                    const int ne = F.load(it, E, flag, sR0);
                    if (!ne || *flag) continue;
                    for (int q = 0; q < ne; q++) {
                        double e[3] = {0, 0, 0}, J[3][6];
                        edge_error<TRANS>(E[q], T, P, e);
                        const double c2 = edge_chi2(E[q], e);
                        double r0 = c2, r1 = 1.0;
                        if (robust) huber(c2, E[q].delta, r0, r1);
                        acc[27] += r0;
                        edge_jacobian<TRANS>(E[q], T, P, J);
                        const int D = E[q].dim;
                        double w[3];
                        for (int i = 0; i < D; i++) w[i] = robust ? r1 * E[q].info[i] : E[q].info[i];
                        int h = 0;
                        for (int k = 0; k < 6; k++) {
                            double s = 0.0;
                            for (int i = 0; i < D; i++) s += (robust ? (r1 * J[i][k]) * E[q].info[i] : J[i][k] * E[q].info[i]) * e[i];
                            acc[21 + k] -= s;
                            for (int l = 0; l <= k; l++, h++) {
                                s = 0.0;
                                for (int i = 0; i < D; i++) s += (J[i][k] * w[i]) * J[i][l];
                                acc[h] += s;
                            }
                        }
                    }
                }
                block_sum(acc, NRED, red, sum);
                if (tid == 0) {
                    int h = 0;
                    for (int k = 0; k < 6; k++) {
                        lm.b[k] = sum[21 + k];
                        for (int l = 0; l <= k; l++, h++) lm.H[k][l] = sum[h];
                    }
                    lm.current = sum[27]; lm.ini = sum[27];
                    if (iter == 0) {                                             // computeLambdaInit
                        double md = 0.0;
                        for (int j = 0; j < 6; j++) md = fabs(lm.H[j][j]) < md ? md : fabs(lm.H[j][j]);
                        lm.lambda = 1e-5 * md; lm.ni = 2.0; lm.nbad = 0;
                        for (int j = 0; j < 6; j++) lm.x[j] = 0.0;
                    }
                }
                int q = 0;
                double rho = 0.0;
                for (;;) {
                    if (tid == 0) {
                        for (int k = 0; k < 6; k++)
                            for (int l = 0; l <= k; l++) lm.M[k][l] = lm.H[k][l] + (k == l ? lm.lambda : 0.0);   // setLambda
                        double xs[6];
                        const bool ok = ldlt_solve(lm.M, lm.b, xs);
                        if (ok) for (int j = 0; j < 6; j++) lm.x[j] = xs[j];
                        sCtl[0] = ok;
                        sTrial = oplus(sT, lm.x);
                    }
                    __syncthreads();
                    double c = 0.0;
                    const SE3 Tt = sTrial;
                    for (int it = tid; it < nItems; it += NT) {
                        const int ne = F.load(it, E, flag, sR0);
                        if (!ne || *flag) continue;
                        for (int k = 0; k < ne; k++) {
                            double e[3] = {0, 0, 0};
                            edge_error<TRANS>(E[k], Tt, P, e);
                            double r0 = edge_chi2(E[k], e), r1;
                            if (robust) huber(r0, E[k].delta, r0, r1);
                            c += r0;
                        }
                    }
                    double tc;
                    block_sum(&c, 1, red, &tc);
                    if (tid == 0) {
                        double temp = tc;
                        if (!sCtl[0]) temp = DBL_MAX;
                        rho = lm.current - temp;
                        double scale = 0.0;
                        for (int j = 0; j < 6; j++) scale += lm.x[j] * (lm.lambda * lm.x[j] + lm.b[j]);
                        scale += 1e-3;
                        rho /= scale;
                        if (rho > 0 && isfinite(temp)) {
                            double alpha = 1. - pow(2 * rho - 1, 3.0);
                            alpha = (2. / 3.) < alpha ? 2. / 3. : alpha;
                            lm.lambda *= (1. / 3.) < alpha ? alpha : 1. / 3.;
                            lm.ni = 2.0;
                            lm.current = temp;
                            sT = sTrial;
                        } else {
                            lm.lambda *= lm.ni;
                            lm.ni *= 2;
                        }
                        q++;
                        const bool again = rho < 0 && q < 10;
                        sCtl[0] = again;
                        if (!again) {
                            bool stop = q == 10 || rho == 0;
                            if (!stop) {                                         // stop criterion (Raul)
                                if ((lm.ini - lm.current) * 1e3 < lm.ini) lm.nbad++;
                                else lm.nbad = 0;
                                stop = lm.nbad >= 3;
                            }
                            sCtl[1] = stop;
                        }
                    }
                    __syncthreads();
                    if (!sCtl[0]) break;
                }
                if (sCtl[1]) break;
            }
        }
        // classification (Optimizer.cc:404-580): an edge flagged last round is evaluated at the estimate, an active one keeps the
        // error of the last trial; both line endpoints are evaluated at the estimate.  TranslationOptimization (:880-1000) treats line
        // endpoints like points (recomputed only when flagged, :943) and does not count bad lines in nBad.
        const SE3 T = sT, Tl = sTrial;
        for (int it = tid; it < nItems; it += NT) {
            const int ne = F.load(it, E, flag, sR0);
            if (!ne) continue;
            bool bad = false;
            if (ne == 2) {
                double e1[3], e2[3];
                const SE3 &Te = TRANS && !*flag ? Tl : T;
                edge_error<TRANS>(E[0], Te, P, e1);
                edge_error<TRANS>(E[1], Te, P, e2);
                const float th = 2 * 5.991f;
                bad = (float)(e1[0] * e1[0]) > th || (float)(e2[0] * e2[0]) > th;
            } else {
                double e[3] = {0, 0, 0};
                edge_error<TRANS>(E[0], *flag ? T : Tl, P, e);
                const float x2 = (float)edge_chi2(E[0], e);
                switch (E[0].kind) {
                case MONO: bad = x2 > 5.991f; break;
                case STEREO: bad = x2 > 7.815f; break;
                case PLANE: bad = (double)x2 > P.prm.plane_chi; break;
                case PAR: case VER: bad = (double)x2 > P.prm.plane_chi_vp; break;
                }
            }
            *flag = bad;
            if (bad && !(TRANS && ne == 2)) atomicAdd(&sCnt[3], 1);
        }
        __syncthreads();
        nbad = sCnt[3];
        if (nEdges < 10) break;
    }
    if (tid == 0) {                                                              // Frame::SetPose(Converter::toCvMat(estimate))
        double R[3][3];
        quat_to_matrix(sT.q, R);
        float *o = P.TcwOut + 12 * (size_t)F.f;
        for (int i = 0; i < 3; i++) {
            o[4 * i] = (float)R[i][0]; o[4 * i + 1] = (float)R[i][1]; o[4 * i + 2] = (float)R[i][2]; o[4 * i + 3] = (float)sT.t[i];
        }
        P.nGood[F.f] = n0 - nbad;
    }
}

}  // namespace

// msl_jacobi.h -- the pinned cyclic Jacobi eigen-solver of a symmetric matrix, stated once (internal).  It stands in for
// cvSVD / cvSolve / cvInvert in msl_pnp.hip and for cv::SVD in msl_line3d.hip and msl_triangulate.hip; tests/pnp_model.py: jacobi_eig is the
// sequential model.  The procedure: JACOBI_SWEEPS sweeps, no convergence branch; a sweep is the round-robin steps of jacobi_pair; a step takes
// the angles of its disjoint pairs from the matrix before the step, then runs all row updates, then all column updates of A and of V; a pair
// with a_pq == 0 is skipped; eigenpairs by descending eigenvalue, the lower index first on ties, no sign normalisation; + - * / sqrt only, in
// double, contraction off.
//   jacobi_pair, jacobi_rotation   the schedule and the rotation of one pair: every driver uses them (msl_pnp.hip's whole-wave LDS driver for
//                                  n <= 12 takes only these and the constant)
//   jacobi_sweep<N>                the register-resident sweep of one thread for n = 3 and n = 4 (msl_line3d.hip, msl_triangulate.hip)
// No memory access, no HIP call: a host program can call the same functions (tests/jacobi_host.cpp).
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MSL_JACOBI_HD __host__ __device__ __forceinline__
#define MSL_JACOBI_UNROLL _Pragma("unroll")
#define MSL_JACOBI_NO_UNROLL _Pragma("unroll 1")
#else
#define MSL_JACOBI_HD inline
#define MSL_JACOBI_UNROLL
#define MSL_JACOBI_NO_UNROLL
#endif

namespace msl {

constexpr int JACOBI_SWEEPS = 16;            // the measurement behind the number

// The round-robin schedule of n indices (padded to the even m = n + (n & 1)): a sweep has m - 1 steps, a step m / 2 slots, each slot a
// pair p < q.  A pair with q >= n holds the padding index and is no pair.
MSL_JACOBI_HD constexpr int jacobi_steps(int n) { return n + (n & 1) - 1; }
MSL_JACOBI_HD constexpr int jacobi_slots(int n) { return (n + (n & 1)) / 2; }
struct JacobiPair { int p, q; };
MSL_JACOBI_HD constexpr JacobiPair jacobi_pair(int n, int step, int slot) {
    const int m = n + (n & 1);
    const int a = slot == 0 ? m - 1 : (step + slot) % (m - 1), b = slot == 0 ? step : (step - slot + m - 1) % (m - 1);
    return JacobiPair{a < b ? a : b, a < b ? b : a};
}

// The rotation (c, s) of the pair with diagonal entries app, aqq and off-diagonal apq; skip: apq == 0, the pair is left as it is.
struct JacobiRot { double c, s; bool skip; };
MSL_JACOBI_HD JacobiRot jacobi_rotation(double app, double aqq, double apq) {
    if (apq == 0) return JacobiRot{1.0, 0.0, true};
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0);
    return JacobiRot{c, t * c, false};
}

// ---- one thread, the matrix in registers ------------------------------------------------------------------------------------------------
// n = 3 and n = 4 have three steps of two slots.  n = 3: slot 0 holds the padding index, so a step is the single pair (1,2), (0,2), (0,1);
// n = 4: the steps are {(0,3),(1,2)}, {(1,3),(0,2)}, {(2,3),(0,1)}.
constexpr bool jacobi_pair_is(int n, int step, int slot, int p, int q) { return jacobi_pair(n, step, slot).p == p && jacobi_pair(n, step, slot).q == q; }
static_assert(jacobi_steps(3) == 3 && jacobi_slots(3) == 2 && jacobi_steps(4) == 3 && jacobi_slots(4) == 2, "three steps of two slots");
static_assert(jacobi_pair(3, 0, 0).q >= 3 && jacobi_pair(3, 1, 0).q >= 3 && jacobi_pair(3, 2, 0).q >= 3, "n = 3: slot 0 is the padding");
static_assert(jacobi_pair_is(3, 0, 1, 1, 2) && jacobi_pair_is(3, 1, 1, 0, 2) && jacobi_pair_is(3, 2, 1, 0, 1), "n = 3: (1,2), (0,2), (0,1)");
static_assert(jacobi_pair_is(4, 0, 0, 0, 3) && jacobi_pair_is(4, 0, 1, 1, 2) && jacobi_pair_is(4, 1, 0, 1, 3) && jacobi_pair_is(4, 1, 1, 0, 2) &&
              jacobi_pair_is(4, 2, 0, 2, 3) && jacobi_pair_is(4, 2, 1, 0, 1), "n = 4: {(0,3),(1,2)}, {(1,3),(0,2)}, {(2,3),(0,1)}");

template <int N, int STEP, int SLOT>
MSL_JACOBI_HD JacobiRot jacobi_slot_angle(const double (&A)[N * N]) {
    constexpr int P = jacobi_pair(N, STEP, SLOT).p, Q = jacobi_pair(N, STEP, SLOT).q;
    if constexpr (Q < N) return jacobi_rotation(A[P * N + P], A[Q * N + Q], A[P * N + Q]);
    else return JacobiRot{1.0, 0.0, true};
}
// The rotation of the slot's pair applied to rows p, q of X (COLS = false) or to its columns p, q (COLS = true)
template <int N, int STEP, int SLOT, bool COLS>
MSL_JACOBI_HD void jacobi_slot_apply(double (&X)[N * N], double c, double s) {
    constexpr int P = jacobi_pair(N, STEP, SLOT).p, Q = jacobi_pair(N, STEP, SLOT).q, SP = COLS ? 1 : N, SK = COLS ? N : 1;
    if constexpr (Q < N) {
        MSL_JACOBI_UNROLL
        for (int k = 0; k < N; k++) {
            const double x = X[P * SP + k * SK], y = X[Q * SP + k * SK];
            X[P * SP + k * SK] = c * x - s * y; X[Q * SP + k * SK] = s * x + c * y;
        }
    }
}
template <int N, int STEP>
MSL_JACOBI_HD void jacobi_step(double (&A)[N * N], double (&V)[N * N]) {
    const JacobiRot r0 = jacobi_slot_angle<N, STEP, 0>(A), r1 = jacobi_slot_angle<N, STEP, 1>(A);
    if (!r0.skip) jacobi_slot_apply<N, STEP, 0, false>(A, r0.c, r0.s);
    if (!r1.skip) jacobi_slot_apply<N, STEP, 1, false>(A, r1.c, r1.s);
    if (!r0.skip) { jacobi_slot_apply<N, STEP, 0, true>(A, r0.c, r0.s); jacobi_slot_apply<N, STEP, 0, true>(V, r0.c, r0.s); }
    if (!r1.skip) { jacobi_slot_apply<N, STEP, 1, true>(A, r1.c, r1.s); jacobi_slot_apply<N, STEP, 1, true>(V, r1.c, r1.s); }
}

// One sweep on the symmetric N x N matrix A, with the same rotations applied to the columns of V.  After JACOBI_SWEEPS sweeps from
// V = identity the diagonal of A holds the eigenvalues and column i of V the eigenvector of A[i][i]; the callers rank them.
template <int N>
MSL_JACOBI_HD void jacobi_sweep(double (&A)[N * N], double (&V)[N * N]) {
    static_assert(N == 3 || N == 4, "three steps of two slots");
    jacobi_step<N, 0>(A, V);
    jacobi_step<N, 1>(A, V);
    jacobi_step<N, 2>(A, V);
}

}  // namespace msl

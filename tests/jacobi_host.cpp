// The pinned Jacobi eigen-solver of manhattanslam_amd/csrc/msl_jacobi.h on the host, against a literal scalar transcription of the pinned
// procedure written here (the generic n <= 12 round-robin schedule of msl_pnp.hip's whole-wave driver, as tests/pnp_model.py: jacobi_eig).
// The register solver is put together as msl_line3d.hip (n = 3) and msl_triangulate.hip (n = 4) put it together: V = identity, JACOBI_SWEEPS
// times jacobi_sweep<N>, ranking by counting.  Eigenvalues and eigenvector rows must agree bit for bit, so the n = 3 and n = 4 pair lists are
// the generic schedule.  Built with -ffp-contract=off -fsanitize=address,undefined by tests/test_jacobi_host.py; exit status 0 = all agree.
#include "msl_jacobi.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }
double uniform(double lo, double hi) { return lo + (hi - lo) * ((double)rnd() / 4294967296.0); }

// ---- the literal transcription: any n <= 12, the matrices in plain arrays, every step as the LDS driver runs it -----------------------------
void literal_eig(int n, const double *A0, double *d, double *ut) {
    double A[144], V[144];
    for (int e = 0; e < n * n; e++) { A[e] = A0[e]; V[e] = (e / n == e % n) ? 1.0 : 0.0; }
    const int m = n + (n & 1), half = m / 2;
    for (int sw = 0; sw < 16; sw++)
        for (int r = 0; r < m - 1; r++) {
            double c[6], s[6]; int jp[6], jq[6];
            for (int lane = 0; lane < half; lane++) {                              // the angles, from the matrix before the step
                const int a = lane == 0 ? m - 1 : (r + lane) % (m - 1), b = lane == 0 ? r : (r - lane + m - 1) % (m - 1);
                int p = a < b ? a : b, q = a < b ? b : a;
                if (q < n) {
                    const double app = A[p * n + p], aqq = A[q * n + q], apq = A[p * n + q];
                    if (apq == 0) {
                        p = -1;
                    } else {
                        const double theta = (aqq - app) / (2.0 * apq);
                        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                        c[lane] = 1.0 / std::sqrt(t * t + 1.0); s[lane] = t * c[lane];
                    }
                } else {
                    p = -1;
                }
                jp[lane] = p; jq[lane] = q;
            }
            for (int pr = 0; pr < half; pr++)                                      // rows p, q of A
                for (int j = 0; j < n; j++) {
                    const int p = jp[pr], q = jq[pr];
                    if (p < 0) continue;
                    const double x = A[p * n + j], y = A[q * n + j];
                    A[p * n + j] = c[pr] * x - s[pr] * y; A[q * n + j] = s[pr] * x + c[pr] * y;
                }
            for (int w = 0; w < 2; w++)                                            // columns p, q of A and of V
                for (int pr = 0; pr < half; pr++)
                    for (int i = 0; i < n; i++) {
                        const int p = jp[pr], q = jq[pr];
                        if (p < 0) continue;
                        double *X = w ? V : A;
                        const double x = X[i * n + p], y = X[i * n + q];
                        X[i * n + p] = c[pr] * x - s[pr] * y; X[i * n + q] = s[pr] * x + c[pr] * y;
                    }
        }
    for (int i = 0; i < n; i++) {                                                  // descending, the lower index first on ties
        int rank = 0;
        for (int j = 0; j < n; j++) { const double dj = A[j * n + j], di = A[i * n + i]; rank += (dj > di || (dj == di && j < i)) ? 1 : 0; }
        d[rank] = A[i * n + i];
        for (int a = 0; a < n; a++) ut[rank * n + a] = V[a * n + i];
    }
}

// ---- the register solver from the header's pieces --------------------------------------------------------------------------------------------
template <int N>
void register_eig(const double *A0, double *d, double *ut) {
    double A[N * N], V[N * N];
    for (int e = 0; e < N * N; e++) { A[e] = A0[e]; V[e] = (e / N == e % N) ? 1.0 : 0.0; }
    for (int sw = 0; sw < msl::JACOBI_SWEEPS; sw++) msl::jacobi_sweep<N>(A, V);
    for (int i = 0; i < N; i++) {
        int rank = 0;
        for (int j = 0; j < N; j++) { const double dj = A[j * N + j], di = A[i * N + i]; rank += (dj > di || (dj == di && j < i)) ? 1 : 0; }
        d[rank] = A[i * N + i];
        for (int a = 0; a < N; a++) ut[rank * N + a] = V[a * N + i];
    }
}

long checked = 0;
int failures = 0;

bool has_nan(const double *x, int n) { for (int i = 0; i < n; i++) if (x[i] != x[i]) return true; return false; }

// nan: the matrix holds a NaN; both solvers must end (they have no convergence branch) and hand the NaN on; the ranks of NaN entries
// collide, so only that is checked
template <int N>
void check(const char *what, const double *A, bool nan = false) {
    double d0[N], u0[N * N], d1[N], u1[N * N];
    std::memset(d0, 0, sizeof d0); std::memset(u0, 0, sizeof u0); std::memset(d1, 0, sizeof d1); std::memset(u1, 0, sizeof u1);
    literal_eig(N, A, d0, u0);
    register_eig<N>(A, d1, u1);
    checked++;
    bool bad;
    if (nan) bad = !(has_nan(d0, N) || has_nan(u0, N * N)) || !(has_nan(d1, N) || has_nan(u1, N * N));
    else bad = std::memcmp(d0, d1, sizeof d0) != 0 || std::memcmp(u0, u1, sizeof u0) != 0;
    if (bad && failures++ < 5) {
        std::fprintf(stderr, "%s (n = %d): literal / register\n", what, N);
        for (int i = 0; i < N; i++) std::fprintf(stderr, "  d[%d] %.17g / %.17g\n", i, d0[i], d1[i]);
        for (int i = 0; i < N * N; i++) std::fprintf(stderr, "  ut[%d] %.17g / %.17g\n", i, u0[i], u1[i]);
    }
}

template <int N>
void symmetric_from(const double *upper, double *A) {   // upper: N (N + 1) / 2 values, row by row
    int e = 0;
    for (int i = 0; i < N; i++)
        for (int j = i; j < N; j++) { A[i * N + j] = upper[e]; A[j * N + i] = upper[e]; e++; }
}

template <int N>
void run_size() {
    double A[N * N], up[N * (N + 1) / 2];
    // fixed-seed symmetric matrices: full range, nearly diagonal, and Gram matrices B^T B (the callers' case)
    for (int i = 0; i < 300; i++) {
        for (double &v : up) v = uniform(-10.0, 10.0);
        symmetric_from<N>(up, A); check<N>("random symmetric", A);
        int e = 0;
        for (int r = 0; r < N; r++) for (int c = r; c < N; c++) up[e++] = r == c ? uniform(0.0, 5.0) : uniform(-1e-6, 1e-6);
        symmetric_from<N>(up, A); check<N>("nearly diagonal", A);
        double B[N * N];
        for (double &v : B) v = uniform(-3.0, 3.0);
        for (int r = 0; r < N; r++) for (int c = 0; c < N; c++) { double s = 0.0; for (int k = 0; k < N; k++) s = s + B[k * N + r] * B[k * N + c]; A[r * N + c] = s; }
        check<N>("Gram matrix", A);
    }
    // diagonal: every pair is skipped; with two equal entries the lower index comes first
    for (int r = 0; r < N; r++) for (int c = 0; c < N; c++) A[r * N + c] = r == c ? (double)(r == 0 ? 2 : r == 1 ? 5 : r == 2 ? 2 : 7) : 0.0;
    check<N>("diagonal with a tie", A);
    for (int r = 0; r < N; r++) for (int c = 0; c < N; c++) A[r * N + c] = r == c ? 1.0 : 0.0;
    check<N>("identity", A);
    std::memset(A, 0, sizeof A);
    check<N>("zero", A);
    // a single zero off-diagonal, in every position
    for (int p = 0; p < N; p++)
        for (int q = p + 1; q < N; q++) {
            for (double &v : up) v = uniform(-4.0, 4.0);
            symmetric_from<N>(up, A);
            A[p * N + q] = 0.0; A[q * N + p] = 0.0;
            check<N>("one zero off-diagonal", A);
        }
    // two equal eigenvalues off the diagonal form: Q diag(3, 3, 1[, 0.5]) Q^T with a plane rotation Q, and the exact 2x2 block [[2, 1], [1, 2]]
    {
        const double lam[4] = {3.0, 3.0, 1.0, 0.5}, cs = std::cos(0.7), sn = std::sin(0.7);
        double Q[N * N];
        for (int r = 0; r < N; r++) for (int c = 0; c < N; c++) Q[r * N + c] = r == c ? 1.0 : 0.0;
        Q[0 * N + 0] = cs; Q[0 * N + 2] = -sn; Q[2 * N + 0] = sn; Q[2 * N + 2] = cs;
        for (int r = 0; r < N; r++) for (int c = r; c < N; c++) { double s = 0.0; for (int k = 0; k < N; k++) s = s + Q[r * N + k] * lam[k] * Q[c * N + k]; A[r * N + c] = s; A[c * N + r] = s; }
        check<N>("two equal eigenvalues", A);
        for (int r = 0; r < N; r++) for (int c = 0; c < N; c++) A[r * N + c] = r == c ? 2.0 : 0.0;
        A[0 * N + 1] = 1.0; A[1 * N + 0] = 1.0;                                    // eigenvalues 3, 1 and the 2s of the other diagonal entries
        check<N>("block with equal diagonal", A);
    }
    // a NaN entry, on and off the diagonal
    for (int k = 0; k < 2; k++) {
        for (double &v : up) v = uniform(-4.0, 4.0);
        symmetric_from<N>(up, A);
        const double nan = std::numeric_limits<double>::quiet_NaN();
        if (k == 0) A[1 * N + 1] = nan; else { A[0 * N + 2] = nan; A[2 * N + 0] = nan; }
        check<N>("NaN entry", A, true);
    }
}

}  // namespace

int main() {
    run_size<3>();
    run_size<4>();
    // rank-deficient A^T A for n = 4 (msl_triangulate's matrix): rows 2 and 3 of the float A are combinations of rows 0 and 1, or equal
    for (int i = 0; i < 100; i++) {
        float Am[16];
        for (int j = 0; j < 8; j++) Am[j] = (float)uniform(-2.0, 2.0);
        const float a = i % 3 == 0 ? 1.0f : (float)uniform(-1.0, 1.0), b = i % 3 == 0 ? 0.0f : (float)uniform(-1.0, 1.0);
        for (int j = 0; j < 4; j++) { Am[8 + j] = a * Am[j] + b * Am[4 + j]; Am[12 + j] = i % 2 ? Am[4 + j] : 0.0f; }
        double G[16];
        for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) { double s = 0.0; for (int k = 0; k < 4; k++) s = s + (double)Am[k * 4 + r] * (double)Am[k * 4 + c]; G[r * 4 + c] = s; }
        check<4>("rank-deficient A^T A", G);
    }
    std::printf("jacobi_host: %ld matrices checked, %d failures\n", checked, failures);
    return failures ? 1 : 0;
}

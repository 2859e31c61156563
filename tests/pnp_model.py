"""Sequential model of msl_pnp_ransac: PnPsolver (reference src/PnPsolver.cc:65-312 and the EPnP it carries, :345-892) with the pins of
INTEGRATION.md section 3j -- the counter-based sampler, the fixed-sweep round-robin Jacobi eigen-solver that stands in for cvSVD / cvSolve /
cvInvert, and left-to-right sums over the correspondences.  NumPy float64 / float32 element-wise arithmetic only (+ - * / sqrt), vectorised
over the hypothesis axis: element-wise array operations round exactly as the scalar ones do."""
import math

import numpy as np

SWEEPS = 16                      # fixed Jacobi sweeps (the measurement behind the number)
PINV_TOL = 1e-12                 # eigenvalues of A^T A at or below PINV_TOL * the largest one are dropped by the pseudo-inverse
M32 = 0xFFFFFFFF
F32, F64 = np.float32, np.float64


# ---- sampling -------------------------------------------------------------------------------------------------------------------------------
def _fmix(h):
    h = h ^ (h >> np.uint64(16)); h = (h * np.uint64(0x85EBCA6B)) & np.uint64(M32)
    h = h ^ (h >> np.uint64(13)); h = (h * np.uint64(0xC2B2AE35)) & np.uint64(M32)
    return h ^ (h >> np.uint64(16))


def hash32(seed, k, j):
    """Draw j of iteration k of a pair with this seed: 32 bits."""
    k = np.asarray(k, np.uint64); j = np.asarray(j, np.uint64)
    h = _fmix(np.uint64(int(seed) & M32) ^ ((k * np.uint64(0x9E3779B1)) & np.uint64(M32)))
    return _fmix(h ^ (((j + np.uint64(1)) * np.uint64(0x85EBCA77)) & np.uint64(M32)))


def sample_sets(seed, K, N, min_set=4):
    """(K, min_set) indices: randi = mulhi32(hash, available), then the swap-with-back removal of PnPsolver.cc:185-190."""
    out = np.zeros((K, min_set), np.int64)
    for k in range(K):
        avail = list(range(N))
        for j in range(min_set):
            r = (int(hash32(seed, k, j)) * len(avail)) >> 32
            out[k, j] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


# ---- SetRansacParameters --------------------------------------------------------------------------------------------------------------------
def ransac_table(N, probability, min_inliers, max_iterations, min_set, epsilon):
    """(mRansacMinInliers, mRansacMaxIts) for N correspondences (PnPsolver.cc:128-147); maxIts is 1 where N < minInliers (no pose, unused)."""
    eps = F32(epsilon)
    n_min = int(F32(N) * eps)
    n_min = max(n_min, min_inliers, min_set)
    if N < n_min:
        return n_min, 1
    if eps < F32(n_min) / F32(N):
        eps = F32(n_min) / F32(N)
    if n_min == N:
        it = 1.0
    else:
        log = lambda x: math.log(x) if x > 0.0 else -math.inf                  # IEEE log(0); inf / nan then flow through the division
        with np.errstate(all="ignore"):
            it = float(np.ceil(F64(log(1.0 - probability)) / F64(log(1.0 - math.pow(float(eps), 3.0)))))
        it = 1.0 if it != it else it                                              # pin: an undefined count is 1
    it = max_iterations if it >= max_iterations else (1 if it < 1 else int(it))
    return n_min, max(1, it)


# ---- the pinned eigen-solver ----------------------------------------------------------------------------------------------------------------
def schedule(n):
    """Round-robin: m - 1 steps of disjoint pairs (p < q), m = n rounded up to even; a pair with the bye index is dropped."""
    m = n + (n & 1)
    steps = []
    for r in range(m - 1):
        pairs = []
        for i in range(m // 2):
            a, b = (m - 1, r) if i == 0 else ((r + i) % (m - 1), (r - i + m - 1) % (m - 1))
            if max(a, b) < n:
                pairs.append((min(a, b), max(a, b)))
        steps.append(pairs)
    return steps


def off_norm(A):
    n = A.shape[-1]
    return np.sqrt(((A * (1 - np.eye(n))) ** 2).sum((-1, -2)))


def jacobi_eig(A, sweeps=SWEEPS, trace=None):
    """Symmetric A (..., n, n) -> (d (..., n) descending, ut (..., n, n) with the eigenvectors as rows).  Each step: the angles of its disjoint
    pairs from the matrix before the step, all row updates, then all column updates; a pair with a_pq == 0 is skipped; no sign normalisation."""
    A = np.array(A, F64)
    n = A.shape[-1]
    V = np.broadcast_to(np.eye(n), A.shape).copy()
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for pairs in schedule(n):
                P = [p for p, _ in pairs]; Q = [q for _, q in pairs]
                app, aqq, apq = A[..., P, P], A[..., Q, Q], A[..., P, Q]
                skip = (apq == 0)[..., None]
                theta = (aqq - app) / (2.0 * apq)
                t = np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = (t * c)[..., None]; c = c[..., None]
                Ap, Aq = A[..., P, :].copy(), A[..., Q, :].copy()
                A[..., P, :] = np.where(skip, Ap, c * Ap - s * Aq)
                A[..., Q, :] = np.where(skip, Aq, s * Ap + c * Aq)
                for X in (A, V):
                    Xp, Xq = np.swapaxes(X[..., :, P], -1, -2).copy(), np.swapaxes(X[..., :, Q], -1, -2).copy()
                    X[..., :, P] = np.swapaxes(np.where(skip, Xp, c * Xp - s * Xq), -1, -2)
                    X[..., :, Q] = np.swapaxes(np.where(skip, Xq, s * Xp + c * Xq), -1, -2)
            if trace is not None:
                trace.append(off_norm(A))
    d = np.diagonal(A, axis1=-2, axis2=-1)
    order = np.argsort(-d, axis=-1, kind="stable")                       # descending, the lower index first on ties
    ut = np.take_along_axis(np.swapaxes(V, -1, -2), order[..., None], axis=-2)
    return np.take_along_axis(d, order, axis=-1), ut


def lapack_eig(A):
    """The same contract from numpy.linalg.eigh (the independent check of the EPnP restatement)."""
    d, V = np.linalg.eigh(A)
    return d[..., ::-1], np.swapaxes(V, -1, -2)[..., ::-1, :]


def _fold(terms, axis):
    """Left-to-right sum from 0.0 along axis."""
    terms = np.moveaxis(np.asarray(terms, F64), axis, 0)
    acc = np.zeros(terms.shape[1:], F64)
    if terms.shape[0] > 64:
        z = np.zeros((1,) + terms.shape[1:], F64)
        return np.add.accumulate(np.concatenate([z, terms], 0), axis=0)[-1]
    for x in terms:
        acc = acc + x
    return acc


def _gram(A):
    """A^T A with every entry a left-to-right sum over the rows."""
    return _fold(A[..., :, :, None] * A[..., :, None, :], -3)


def _inv_eigs(d):
    with np.errstate(all="ignore"):
        return np.where(d > d[..., :1] * PINV_TOL, 1.0 / d, 0.0)


def pinv_solve(A, b, eig):
    """cvSolve(A, b, x, CV_SVD): x = V diag(1/d) V^T A^T b over the eigenpairs (d, V) of A^T A."""
    d, ut = eig(_gram(A))
    atb = _fold(A * b[..., :, None], -2)
    y = _fold(ut * atb[..., None, :], -1) * _inv_eigs(d)
    return _fold(ut * y[..., :, None], -2)


def pinv3(A, eig):
    """cvInvert(A, inv, CV_SVD) for a 3x3."""
    d, ut = eig(_gram(A))
    B = _fold(ut[..., :, :, None] * np.swapaxes(A, -1, -2)[..., None, :, :], -2) * _inv_eigs(d)[..., None]     # B[j][c] = sum_a V[a][j] A[c][a]
    return _fold(ut[..., :, :, None] * B[..., :, None, :], -3)                                                   # inv[r][c] = sum_j V[r][j] B[j][c]


def rot_from_abt(A, eig):
    """U V^T of cvSVD(ABt): V, d from A^T A, U[:, k] = A V[:, k] / sqrt(d_k)."""
    d, ut = eig(_gram(A))
    with np.errstate(all="ignore"):
        U = _fold(A[..., :, None, :] * ut[..., None, :, :], -1) / np.sqrt(d)[..., None, :]                       # U[i][k] = sum_a A[i][a] V[a][k]
    return _fold(U[..., :, None, :] * np.swapaxes(ut, -1, -2)[..., None, :, :], -1)                              # R[i][j] = sum_k U[i][k] V[j][k]


# ---- EPnP (PnPsolver.cc:345-892) ------------------------------------------------------------------------------------------------------------
def _dot3(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _qr_solve(A, b, x_prev):
    """The file's Householder qr_solve (:803-892) on (H, 6, 4): its row scan stops one row short, and a zero column leaves X as it was."""
    A = A.copy(); b = b.copy()
    H = A.shape[0]; nr, nc = 6, 4
    A1 = np.zeros((H, nc)); A2 = np.zeros((H, nc))
    dead = np.zeros(H, bool)
    for k in range(nc):
        eta = np.abs(A[:, k, k])
        for i in range(k, nr - 1):
            eta = np.where(eta < np.abs(A[:, i, k]), np.abs(A[:, i, k]), eta)
        dead |= eta == 0
        inv_eta = 1.0 / eta
        s = np.zeros(H)
        for i in range(k, nr):
            A[:, i, k] = A[:, i, k] * inv_eta
            s = s + A[:, i, k] * A[:, i, k]
        sigma = np.sqrt(s)
        sigma = np.where(A[:, k, k] < 0, -sigma, sigma)
        A[:, k, k] = A[:, k, k] + sigma
        A1[:, k] = sigma * A[:, k, k]
        A2[:, k] = -eta * sigma
        for j in range(k + 1, nc):
            s = np.zeros(H)
            for i in range(k, nr):
                s = s + A[:, i, k] * A[:, i, j]
            tau = s / A1[:, k]
            for i in range(k, nr):
                A[:, i, j] = A[:, i, j] - tau * A[:, i, k]
    for j in range(nc):
        tau = np.zeros(H)
        for i in range(j, nr):
            tau = tau + A[:, i, j] * b[:, i]
        tau = tau / A1[:, j]
        for i in range(j, nr):
            b[:, i] = b[:, i] - tau * A[:, i, j]
    x = np.zeros((H, nc))
    x[:, nc - 1] = b[:, nc - 1] / A2[:, nc - 1]
    for i in range(nc - 2, -1, -1):
        s = np.zeros(H)
        for j in range(i + 1, nc):
            s = s + A[:, i, j] * x[:, j]
        x[:, i] = (b[:, i] - s) / A2[:, i]
    return np.where(dead[:, None], x_prev, x)


def _gauss_newton(L, rho, betas):
    betas = betas.copy()
    x = np.zeros_like(betas)                                             # pin: X starts as zeros (the reference leaves it uninitialised)
    b0, b1, b2, b3 = (betas[:, i] for i in range(4))
    for _ in range(5):
        b0, b1, b2, b3 = (betas[:, i] for i in range(4))
        l = [L[:, :, i] for i in range(10)]
        A = np.stack([2 * l[0] * b0[:, None] + l[1] * b1[:, None] + l[3] * b2[:, None] + l[6] * b3[:, None],
                      l[1] * b0[:, None] + 2 * l[2] * b1[:, None] + l[4] * b2[:, None] + l[7] * b3[:, None],
                      l[3] * b0[:, None] + l[4] * b1[:, None] + 2 * l[5] * b2[:, None] + l[8] * b3[:, None],
                      l[6] * b0[:, None] + l[7] * b1[:, None] + l[8] * b2[:, None] + 2 * l[9] * b3[:, None]], -1)
        B0, B1, B2, B3 = b0[:, None], b1[:, None], b2[:, None], b3[:, None]
        bb = rho - (l[0] * B0 * B0 + l[1] * B0 * B1 + l[2] * B1 * B1 + l[3] * B0 * B2 + l[4] * B1 * B2 + l[5] * B2 * B2 + l[6] * B0 * B3 +
                    l[7] * B1 * B3 + l[8] * B2 * B3 + l[9] * B3 * B3)
        x = _qr_solve(A, bb, x)
        betas = betas + x
    return betas


def compute_pose(pws, us, K, eig=jacobi_eig, details=None):
    """PnPsolver::compute_pose for H independent sets of n correspondences: pws (H, n, 3), us (H, n, 2) float64, K = (fu, fv, uc, vc).
    Returns R (H, 3, 3), t (H, 3), branch (H,) in 1..3, rep_error (H,)."""
    pws = np.asarray(pws, F64); us = np.asarray(us, F64)
    fu, fv, uc, vc = (F64(v) for v in K)
    H, n = pws.shape[:2]
    with np.errstate(all="ignore"):
        # choose_control_points
        c0 = _fold(pws, 1) / n
        pw0 = pws - c0[:, None, :]
        dc, uct = eig(_gram(pw0))
        kk = np.sqrt(np.where(dc > 0, dc, 0.0) / n)
        cws = np.concatenate([c0[:, None, :], c0[:, None, :] + kk[:, :, None] * uct], 1)                          # (H, 4, 3)
        # compute_barycentric_coordinates
        cc = np.swapaxes(cws[:, 1:, :] - cws[:, :1, :], 1, 2)                                                     # cc[i][j-1] = cws[j][i] - cws[0][i]
        ci = pinv3(cc, eig)
        dp = pws - cws[:, :1, :]
        a123 = ci[:, None, :, 0] * dp[:, :, None, 0] + ci[:, None, :, 1] * dp[:, :, None, 1] + ci[:, None, :, 2] * dp[:, :, None, 2]   # (H, n, 3)
        a0 = 1.0 - a123[..., 0] - a123[..., 1] - a123[..., 2]
        al = np.concatenate([a0[..., None], a123], -1)                                                            # (H, n, 4)
        # fill_M, MtM
        z = np.zeros_like(al)
        du, dv = (uc - us[..., 0])[..., None], (vc - us[..., 1])[..., None]
        M1 = np.stack([al * fu, z, al * du], -1).reshape(H, n, 12)
        M2 = np.stack([z, al * fv, al * dv], -1).reshape(H, n, 12)
        M = np.stack([M1, M2], 2).reshape(H, 2 * n, 12)
        _, ut = eig(_gram(M))
        if details is not None:
            details["ut"] = ut
        # compute_L_6x10, compute_rho
        v = [ut[:, 11 - i].reshape(H, 4, 3) for i in range(4)]
        ab = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
        dvv = [[v[i][:, a] - v[i][:, b] for a, b in ab] for i in range(4)]
        L = np.zeros((H, 6, 10))
        for i in range(6):
            d0, d1, d2, d3 = dvv[0][i], dvv[1][i], dvv[2][i], dvv[3][i]
            L[:, i] = np.stack([_dot3(d0, d0), 2.0 * _dot3(d0, d1), _dot3(d1, d1), 2.0 * _dot3(d0, d2), 2.0 * _dot3(d1, d2), _dot3(d2, d2),
                                2.0 * _dot3(d0, d3), 2.0 * _dot3(d1, d3), 2.0 * _dot3(d2, d3), _dot3(d3, d3)], -1)
        rho = np.stack([_dot3(cws[:, a] - cws[:, b], cws[:, a] - cws[:, b]) for a, b in ab], -1)
        # the three beta initialisations
        betas = []
        b4 = pinv_solve(L[:, :, [0, 1, 3, 6]], rho, eig)
        neg = b4[:, 0] < 0
        be0 = np.sqrt(np.where(neg, -b4[:, 0], b4[:, 0]))
        sg = np.where(neg, -1.0, 1.0)
        betas.append(np.stack([be0, sg * b4[:, 1] / be0, sg * b4[:, 2] / be0, sg * b4[:, 3] / be0], -1))
        for cols in ([0, 1, 2], [0, 1, 2, 3, 4]):
            b = pinv_solve(L[:, :, cols], rho, eig)
            neg = b[:, 0] < 0
            be0 = np.sqrt(np.where(neg, -b[:, 0], b[:, 0]))
            be1 = np.where(neg, np.where(b[:, 2] < 0, np.sqrt(-b[:, 2]), 0.0), np.where(b[:, 2] > 0, np.sqrt(b[:, 2]), 0.0))
            be0 = np.where(b[:, 1] < 0, -be0, be0)
            be2 = b[:, 3] / be0 if len(cols) == 5 else np.zeros(H)
            betas.append(np.stack([be0, be1, be2, np.zeros(H)], -1))
        Rs, ts, errs = [], [], []
        pw_mean = _fold(pws, 1) / n
        for be in betas:
            be = _gauss_newton(L, rho, be)
            # compute_ccs, compute_pcs, solve_for_sign
            ccs = np.zeros((H, 4, 3))
            for i in range(4):
                ccs = ccs + be[:, i, None, None] * ut[:, 11 - i].reshape(H, 4, 3)
            flip = (al[:, 0, 0] * ccs[:, 0, 2] + al[:, 0, 1] * ccs[:, 1, 2] + al[:, 0, 2] * ccs[:, 2, 2] + al[:, 0, 3] * ccs[:, 3, 2]) < 0.0
            ccs = np.where(flip[:, None, None], -ccs, ccs)
            pcs = al[..., 0, None] * ccs[:, None, 0] + al[..., 1, None] * ccs[:, None, 1] + al[..., 2, None] * ccs[:, None, 2] + \
                al[..., 3, None] * ccs[:, None, 3]                                                                # (H, n, 3)
            # estimate_R_and_t
            pc0 = _fold(pcs, 1) / n
            abt = _fold((pcs - pc0[:, None])[..., :, None] * (pws - pw_mean[:, None])[..., None, :], 1)
            R = rot_from_abt(abt, eig)
            det = R[:, 0, 0] * R[:, 1, 1] * R[:, 2, 2] + R[:, 0, 1] * R[:, 1, 2] * R[:, 2, 0] + R[:, 0, 2] * R[:, 1, 0] * R[:, 2, 1] - \
                R[:, 0, 2] * R[:, 1, 1] * R[:, 2, 0] - R[:, 0, 1] * R[:, 1, 0] * R[:, 2, 2] - R[:, 0, 0] * R[:, 1, 2] * R[:, 2, 1]
            R = R.copy()
            R[:, 2] = np.where((det < 0)[:, None], -R[:, 2], R[:, 2])
            t = np.stack([pc0[:, i] - _dot3(R[:, i], pw_mean) for i in range(3)], -1)
            # reprojection_error
            Xc = _dot3(R[:, None, 0], pws) + t[:, None, 0]
            Yc = _dot3(R[:, None, 1], pws) + t[:, None, 1]
            iz = 1.0 / (_dot3(R[:, None, 2], pws) + t[:, None, 2])
            ue = uc + fu * Xc * iz
            ve = vc + fv * Yc * iz
            err = _fold(np.sqrt((us[..., 0] - ue) * (us[..., 0] - ue) + (us[..., 1] - ve) * (us[..., 1] - ve)), 1) / n
            Rs.append(R); ts.append(t); errs.append(err)
        branch = np.ones(H, np.int64)
        branch = np.where(errs[1] < errs[0], 2, branch)
        cur = np.where(branch == 2, errs[1], errs[0])
        branch = np.where(errs[2] < cur, 3, branch)
    sel = branch[:, None, None]
    R = np.where(sel == 1, Rs[0], np.where(sel == 2, Rs[1], Rs[2]))
    t = np.where(sel[:, 0] == 1, ts[0], np.where(sel[:, 0] == 2, ts[1], ts[2]))
    err = np.where(branch == 1, errs[0], np.where(branch == 2, errs[1], errs[2]))
    return R, t, branch, err


def check_inliers(R, t, p3d, p2d, max_err, K):
    """PnPsolver::CheckInliers (:286-312) with its float / double mix.  R (H, 3, 3), t (H, 3) float64; p3d, p2d, max_err float32.
    Returns (inlier (H, N) bool, margin: the smallest |error2 - maxError| / maxError met)."""
    fu, fv, uc, vc = (F64(v) for v in K)
    X = np.asarray(p3d, F32).astype(F64)
    with np.errstate(all="ignore"):
        def row(i):
            return R[:, i, 0, None] * X[None, :, 0] + R[:, i, 1, None] * X[None, :, 1] + R[:, i, 2, None] * X[None, :, 2] + t[:, i, None]
        Xc = row(0).astype(F32); Yc = row(1).astype(F32)
        iz = (1.0 / row(2)).astype(F32)
        ue = uc + fu * Xc.astype(F64) * iz.astype(F64)
        ve = vc + fv * Yc.astype(F64) * iz.astype(F64)
        dx = (p2d[None, :, 0].astype(F64) - ue).astype(F32)
        dy = (p2d[None, :, 1].astype(F64) - ve).astype(F32)
        e2 = dx * dx + dy * dy
        inl = e2 < max_err[None, :]
        m = np.abs(e2.astype(F64) - max_err[None, :].astype(F64)) / max_err[None, :].astype(F64)
    m = m[np.isfinite(m)]
    return inl, (float(m.min()) if m.size else np.inf)


# ---- one complete run -----------------------------------------------------------------------------------------------------------------------
def gather(params, octave, un_xy, match, xyz):
    """The correspondences of PnPsolver.cc:76-96: valid matches in ascending keypoint order."""
    kcap = len(xyz)
    match = np.asarray(match)
    kp = np.nonzero((match >= 0) & (match < kcap))[0]
    nl = int(params["nlevels"])
    oc = np.clip(np.asarray(octave)[kp], 0, nl - 1)
    sigma2 = np.asarray(params["level_sigma2"], F32).reshape(-1)[oc]
    return kp, np.asarray(un_xy, F32)[kp], np.asarray(xyz, F32)[match[kp]], (sigma2 * F32(params["th2"])).astype(F32)


def pnp_ransac(params, octave, un_xy, match, xyz, seed, eig=jacobi_eig, literal=False):
    """One iterate(n_iterations) of a fresh PnPsolver.  params: a dict with the fields of msl_pnp_params.  literal: Refine at every qualifying
    iteration exactly as :199-224 does, instead of at records only.  Returns a dict of the outputs and the per-hypothesis stage."""
    g = lambda k: params[k][0] if isinstance(params[k], np.ndarray) and params[k].shape == (1,) else params[k]
    K = (g("fx"), g("fy"), g("cx"), g("cy"))
    n_kps = len(match)
    kp, p2d, p3d, max_err = gather({"nlevels": g("nlevels"), "level_sigma2": g("level_sigma2"), "th2": g("th2")}, octave, un_xy, match, xyz)
    N = len(kp)
    min_inl, max_its = ransac_table(N, float(g("probability")), int(g("min_inliers")), int(g("max_iterations")), int(g("min_set")), g("epsilon"))
    out = dict(status=0, n_inliers=0, inlier=np.zeros(n_kps, np.uint8), pt_ref=np.full(n_kps, -1, np.int32),
               Tcw=np.eye(4, dtype=F32)[:3].copy(), N=N, min_inliers=min_inl, K=0, margin=np.inf, first_success=-1, refines=0,
               R=np.zeros((0, 3, 3)), t=np.zeros((0, 3)), branch=np.zeros(0, np.int64), count=np.zeros(0, np.int64))
    if N < min_inl:
        return out
    Kit = max(max_its, int(g("n_iterations")))
    sets = sample_sets(seed, Kit, N)
    R, t, branch, _ = compute_pose(p3d[sets].astype(F64), p2d[sets].astype(F64), K, eig)
    inl, margin = check_inliers(R, t, p3d, p2d, max_err, K)
    count = inl.sum(1)
    out.update(K=Kit, R=R, t=t, branch=branch, count=count)
    best = 0; best_k = -1; result = None

    def refine(mask):
        nonlocal margin
        idx = np.nonzero(mask)[0]
        Rr, tr, _, _ = compute_pose(p3d[idx].astype(F64)[None], p2d[idx].astype(F64)[None], K, eig)
        ri, m = check_inliers(Rr, tr, p3d, p2d, max_err, K)
        margin = min(margin, m)
        out["refines"] += 1
        return Rr[0], tr[0], ri[0]

    for k in range(Kit):
        if count[k] < min_inl:
            continue
        record = count[k] > best
        if record:
            best, best_k = int(count[k]), k
        if record or literal:
            Rr, tr, ri = refine(inl[best_k])
            if ri.sum() > min_inl:
                result = (1, Rr, tr, ri); out["first_success"] = k
                break
    if result is None and best_k >= 0:
        result = (2, R[best_k], t[best_k], inl[best_k])
    out["margin"] = margin
    if result is not None:
        st, Ro, to, mask = result
        out["status"] = st; out["n_inliers"] = int(mask.sum())
        out["inlier"][kp[mask]] = 1
        out["pt_ref"] = np.where(out["inlier"] != 0, np.asarray(match, np.int32), np.int32(-1)).astype(np.int32)
        out["Tcw"] = np.concatenate([Ro.astype(F32), to.astype(F32)[:, None]], 1)
    return out

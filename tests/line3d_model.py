"""Sequential model of msl_lines_3d: Frame::GetLineDepth (reference src/Frame.cc:179-186), Frame::Obtain3DLine (:528-603) with all of
src/3DLineExtractor.cpp, and the line half of the three call sites (src/Tracking.cc:575-592, :1107-1143, :1569-1618), restated statement by
statement with the pins of DESIGN.md section 3 / INTEGRATION.md section 3k.  Python floats are IEEE doubles, numpy.float32 scalars the
reference's floats.  The only array arithmetic is element-wise over the samples of one keyline (their covariance, DU and Mahalanobis
distance are independent per sample), which rounds exactly as the scalar statements do; every sum over samples is an explicit loop."""
import math

import numpy as np

from tests.local_match_model import gemm3
from tests.pnp_model import hash32, jacobi_eig

F32, F64 = np.float32, np.float64
ALL, INDEX_ORDER, DEPTH_ORDER = 0, 1, 2
EPS = 1e-10


def default_params(fx=525.0, fy=525.0, cx=319.5, cy=239.5, **kw):
    p = dict(fx=fx, fy=fy, cx=cx, cy=cy, max_samples=100, min_points=10, max_iterations=10, max_new_lines=30, dist_thresh=1.5,
             min_support=0.4, min_length=0.02)
    p.update(kw)
    return p


# ---- Frame::GetLineDepth ------------------------------------------------------------------------------------------------------------------
def _trunc(v):
    """float -> int as the C conversion does; None where it is undefined (the pin: such an end point has no depth)."""
    v = float(v)
    return int(v) if math.isfinite(v) and abs(v) < 2147483648.0 else None


def end_depth(depth, x, y):
    """imDepth.at<float>(y, x) with the truncating conversion; pin: -1.0f outside the image (the reference reads unchecked)."""
    r, c = _trunc(y), _trunc(x)
    if r is None or c is None or r < 0 or c < 0 or r >= depth.shape[0] or c >= depth.shape[1]:
        return F32(-1.0)
    return F32(depth[r, c])


# ---- 3DLineExtractor.cpp ------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _norm(a):
    return math.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def _mul(a, s):
    return (a[0] * s, a[1] * s, a[2] * s)


def depth_std_dev(d):
    return 0.00273 * d * d + 0.00074 * d + -0.00058


def cov0_of(pos, fx):
    """compPt3dCov's cov0 = J0 diag(1, 1, sigma(z)^2) J0^T for samples pos (n, 3): the products of the two matrix multiplications without
    their exact zero terms, f = fx for both rows; the symmetric matrix is taken from the upper triangle."""
    x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
    f = F64(fx)
    with np.errstate(all="ignore"):
        s = depth_std_dev(z)
        s2 = s * s
        a = z / f; bx = x / z; by = y / z
        mx = bx * s2; my = by * s2                       # (J0 cov_g)[0][2], [1][2]
        c = np.zeros((len(pos), 3, 3), F64)
        c[:, 0, 0] = a * a + mx * bx; c[:, 0, 1] = mx * by; c[:, 0, 2] = mx
        c[:, 1, 1] = a * a + my * by; c[:, 1, 2] = my
        c[:, 2, 2] = s2
        c[:, 1, 0] = c[:, 0, 1]; c[:, 2, 0] = c[:, 0, 2]; c[:, 2, 1] = c[:, 1, 2]
    return c


def du_of(cov, eig=jacobi_eig):
    """DU = diag(1 / sqrt(w)) U^T from the eigenpairs of cov0 (pin: the project's Jacobi solver stands in for cv::SVD)."""
    d, ut = eig(cov)
    with np.errstate(all="ignore"):
        return (1.0 / np.sqrt(d))[:, :, None] * ut


def mah_dist(pos, DU, q1, q2):
    """mah_dist3d_pt_line of every sample against the line (q1, q2), in the file's operation order."""
    xa, ya, za = q1; xb, yb, zb = q2
    c1, c2, c3, c4, c5, c6, c7, c8, c9 = (DU[:, i, j] for i in range(3) for j in range(3))
    x1, x2, x3 = pos[:, 0], pos[:, 1], pos[:, 2]
    with np.errstate(all="ignore"):
        term1 = ((c1 * (x1 - xa) + c2 * (x2 - ya) + c3 * (x3 - za)) * (c4 * (x1 - xb) + c5 * (x2 - yb) + c6 * (x3 - zb))
                 - (c4 * (x1 - xa) + c5 * (x2 - ya) + c6 * (x3 - za)) * (c1 * (x1 - xb) + c2 * (x2 - yb) + c3 * (x3 - zb)))
        term2 = ((c1 * (x1 - xa) + c2 * (x2 - ya) + c3 * (x3 - za)) * (c7 * (x1 - xb) + c8 * (x2 - yb) + c9 * (x3 - zb))
                 - (c7 * (x1 - xa) + c8 * (x2 - ya) + c9 * (x3 - za)) * (c1 * (x1 - xb) + c2 * (x2 - yb) + c3 * (x3 - zb)))
        term3 = ((c4 * (x1 - xa) + c5 * (x2 - ya) + c6 * (x3 - za)) * (c7 * (x1 - xb) + c8 * (x2 - yb) + c9 * (x3 - zb))
                 - (c7 * (x1 - xa) + c8 * (x2 - ya) + c9 * (x3 - za)) * (c4 * (x1 - xb) + c5 * (x2 - yb) + c6 * (x3 - zb)))
        term4 = c1 * (x1 - xa) - c1 * (x1 - xb) + c2 * (x2 - ya) - c2 * (x2 - yb) + c3 * (x3 - za) - c3 * (x3 - zb)
        term5 = c4 * (x1 - xa) - c4 * (x1 - xb) + c5 * (x2 - ya) - c5 * (x2 - yb) + c6 * (x3 - za) - c6 * (x3 - zb)
        term6 = c7 * (x1 - xa) - c7 * (x1 - xb) + c8 * (x2 - ya) - c8 * (x2 - yb) + c9 * (x3 - za) - c9 * (x3 - zb)
        return np.sqrt((term1 * term1 + term2 * term2 + term3 * term3) / (term4 * term4 + term5 * term5 + term6 * term6))


def _project(P, mid, drct):
    """projectPt3d2Ln3d"""
    A = mid
    B = _add(mid, drct)
    AB = _sub(B, A)
    AP = _sub(P, A)
    return _add(A, _mul(AB, _dot(AB, AP) / _dot(AB, AB)))


def _extremes(pts, idx, origin, direction):
    """The minv = 100 / maxv = -100 scan both verify3dLine and the end-point search run: positions in idx of the two extremes."""
    minv, maxv, i1, i2 = 100.0, -100.0, 0, 0
    for i, s in enumerate(idx):
        v = _dot(_sub(pts[s], origin), direction)
        if v < minv:
            minv, i1 = v, i
        if v > maxv:
            maxv, i2 = v, i
    return i1, i2


def verify_3d_line(pts, idx, A, B, margins):
    AB = _sub(B, A)
    i1, i2 = _extremes(pts, idx, A, AB)
    mid = _mul(_add(A, B), 0.5)
    C = _project(pts[idx[i1]], mid, AB)
    D = _project(pts[idx[i2]], mid, AB)
    DC = _sub(D, C)
    cd = _norm(DC)
    if cd < EPS:
        return False
    cells = [0] * 10
    for s in idx:
        lam = abs(_dot(_sub(pts[s], C), DC) / cd / cd)
        if lam >= 1:
            cells[9] += 1
        else:
            cells[int(math.floor(lam * 10))] += 1
        # the decision changes at lam * 10 = 1 .. 9 only: |.| folds everything below 0 into cell 0, and [9, 10) and [10, inf) share the last cell
        margins["cell"] = min(margins["cell"], min(abs(lam * 10 - k) for k in range(1, 10)))
    occupied = 0.0
    for c in cells:
        if c > 0:
            occupied = occupied + 1
    return occupied / 10 > 0.7


def _inliers(pos, DU, q1, q2, th, margins):
    dist = mah_dist(pos, DU, q1, q2)
    fin = dist[np.isfinite(dist)]
    if fin.size:
        margins["dist"] = min(margins["dist"], float(np.min(np.abs(fin - th) / th)))
    with np.errstate(all="ignore"):
        return [int(i) for i in np.nonzero(dist < th)[0]]                # a NaN distance is not an inlier


def refit_sums(pts, idx):
    """computeLine3d_svd up to the decomposition: the mean (left-to-right sum times 1.0 / n) and P^T P of the centred points (left-to-right
    sums over idx in order)."""
    n = len(idx)
    mean = (0.0, 0.0, 0.0)
    for s in idx:
        mean = _add(mean, pts[s])
    mean = _mul(mean, 1.0 / n)
    G = np.zeros((3, 3), F64)
    for s in idx:
        c = _sub(pts[s], mean)
        for a in range(3):
            for b in range(3):
                G[a, b] = G[a, b] + c[a] * c[b]
    return mean, G


def extract_3d_line(pos, DU, seed, prm, eig=jacobi_eig, margins=None):
    """extract3dline_mahdist: (inlier sample indices, A, B, trace)."""
    margins = margins if margins is not None else dict(dist=math.inf, cell=math.inf)
    n = len(pos)
    pts = [tuple(float(v) for v in p) for p in pos]
    th = float(prm["dist_thresh"])
    max_iter = min(int(prm["max_iterations"]), int(n * (n - 1) * 0.5))
    indexes = list(range(n))
    best, best_a, best_b = [], None, None
    iters = []
    for it in range(max_iter):
        begin, left = 0, n
        for j in range(2):                                               # random_unique(indexes, 2); pin: rand() % left -> mulhi32(hash, left)
            r = (int(hash32(seed, it, j)) * left) >> 32
            indexes[begin], indexes[begin + r] = indexes[begin + r], indexes[begin]
            begin += 1; left -= 1
        ia, ib = indexes[0], indexes[1]
        A, B = pts[ia], pts[ib]
        if _norm(_sub(B, A)) < EPS:
            iters.append((ia, ib, -1, 0))
            continue
        inl = _inliers(pos, DU, A, B, th, margins)
        record = 0
        if len(inl) > len(best):
            if verify_3d_line(pts, inl, A, B, margins):
                best, best_a, best_b, record = inl, A, B, 1
        iters.append((ia, ib, len(inl), record))
        if len(best) > n * 0.6:
            break
    trace = dict(iters=iters, refits=0, m=(0.0, 0.0, 0.0), d=(0.0, 0.0, 0.0), ends=(0, 0), gram=[])
    A = B = (0.0, 0.0, 0.0)
    if len(best) >= 2:
        m, d = _mul(_add(best_a, best_b), 0.5), _sub(best_b, best_a)
        while True:
            trace["refits"] += 1
            tm, G = refit_sums(pts, best)
            trace["gram"].append((tm, G.copy(), list(best)))
            td = tuple(float(v) for v in eig(G)[1][0])                   # pin: the first right singular vector = the top eigenvector of P^T P
            tmp = _inliers(pos, DU, tm, _add(tm, td), th, margins)
            if len(tmp) > len(best):
                best, m, d = tmp, tm, td
            else:
                break
        i1, i2 = _extremes(pts, best, m, d)
        trace.update(m=m, d=d, ends=(best[i1], best[i2]))
        A, B = pts[best[i1]], pts[best[i2]]
    return best, A, B, trace


# ---- Frame::Obtain3DLine ------------------------------------------------------------------------------------------------------------------
def sample_pixels(ends, shape, prm):
    """The sampling loop of Obtain3DLine up to the depth look-up: (len, [(row, col)] of the samples inside the image, in order)."""
    sx, sy, ex, ey = (F32(v) for v in ends)
    dx, dy = sx - ex, sy - ey
    ln = math.sqrt(float(dx) * float(dx) + float(dy) * float(dy))
    if not math.isfinite(ln):
        return ln, []
    num = min(int(ln), int(prm["max_samples"]))
    rows, cols = shape
    out = []
    if num == 0:                                                         # pin: j / numSmp divides by zero -> no line
        return ln, out
    num_d = float(num)
    for j in range(num + 1):
        t = j / num_d
        a = 1 - t
        px = F32(float(sx) * a) + F32(float(ex) * t)                     # Point2f * double rounds to float; the sum is a float sum
        py = F32(float(sy) * a) + F32(float(ey) * t)
        x, y = float(px), float(py)
        if not (x >= 0 and y >= 0 and x < cols and y < rows):            # `pt.x < 0 || ... continue`; a NaN position is dropped too (pin)
            continue
        if math.floor(x) == x and math.floor(y) == y:
            col = max(int(x - 1), 0); row = max(int(y - 1), 0)
        else:
            col = int(x); row = int(y)
        out.append((row, col))
    return ln, out


def sample_points(ends, depth, prm):
    """The sampling loop of Obtain3DLine: (len, positions (n, 3) float64)."""
    fx, fy, cx, cy = (F32(prm[k]) for k in ("fx", "fy", "cx", "cy"))
    invfx, invfy = F32(1.0) / fx, F32(1.0) / fy
    ln, pix = sample_pixels(ends, depth.shape, prm)
    out = []
    for row, col in pix:
        d = F32(depth[row, col])
        if float(d) <= 0.01:                                             # float against the double literal
            continue
        z = float(d)
        out.append((float(F32(col) - cx) * z * float(invfx), float(F32(row) - cy) * z * float(invfy), z))
    return ln, np.array(out, F64).reshape(-1, 3)


def obtain_3d_line(ends, depth, Tcw, seed, prm, eig=jacobi_eig, sampled=None):
    """Frame::Obtain3DLine for one keyline: dict(ok, xyz (6,) float64, n_support, n_kept, trace, margins, pos, DU).  sampled: (len, pos, DU)
    when the caller has run the sampling loop and compPt3dCov already (lines_3d does, for all keylines of a frame in one array)."""
    margins = dict(dist=math.inf, cell=math.inf, support=math.inf, length=math.inf)
    ln, pos, DU = sampled if sampled is not None else sample_points(ends, depth, prm) + (None,)
    out = dict(ok=0, xyz=np.zeros(6, F64), n_support=0, n_kept=len(pos), len=ln, margins=margins, pos=pos, DU=None,
               trace=dict(iters=[], refits=0, m=(0.0, 0.0, 0.0), d=(0.0, 0.0, 0.0), ends=(0, 0), gram=[]))
    if len(pos) < int(prm["min_points"]):
        return out
    if DU is None:
        DU = du_of(cov0_of(pos, F32(prm["fx"])), eig)
    best, A, B, trace = extract_3d_line(pos, DU, seed, prm, eig, margins)
    out.update(DU=DU, trace=trace, n_support=len(best), inliers=best)
    ratio, length = len(best) / ln, _norm(_sub(A, B))
    ms, ml = float(prm["min_support"]), float(prm["min_length"])
    if best:
        margins["support"] = abs(ratio - ms) / ms
        margins["length"] = abs(length - ml) / ml
    if ratio > ms and length > ml:
        T = np.asarray(Tcw, F32).reshape(3, 4)
        Ow = gemm3(T, True, -1.0, T[:, 3])                                # mOw = -mRcw.t() * mtcw
        Aw = gemm3(T, True, 1.0, np.array(A, F64).astype(F32), Ow)         # mRwc * Ac + mOw
        Bw = gemm3(T, True, 1.0, np.array(B, F64).astype(F32), Ow)
        out.update(ok=1, xyz=np.concatenate([Aw, Bw]).astype(F64))
    return out


# ---- the call sites -----------------------------------------------------------------------------------------------------------------------
def select(order, depth_pairs, flags, ok, max_new_lines):
    """line_new of one frame from the per-keyline results: candidates are walked in the call site's order with its stop."""
    n = len(depth_pairs)
    new = np.zeros(n, np.uint8)
    both = [float(depth_pairs[i][0]) > 0 and float(depth_pairs[i][1]) > 0 for i in range(n)]
    if order == ALL:
        for i in range(n):
            new[i] = 1 if both[i] and ok[i] else 0
        return new
    walk = [i for i in range(n) if both[i]]
    if order == DEPTH_ORDER:
        walk.sort(key=lambda i: (float(min(F32(depth_pairs[i][0]), F32(depth_pairs[i][1]))), i))
    count = 0
    for i in walk:
        if (int(flags[i]) & 3) == 3:
            count += 1
        elif ok[i]:
            new[i] = 1; count += 1
        else:
            continue
        if count > max_new_lines:
            break
    return new


def lines_3d(order, prm, line_ends, depth, flags, Tcw, seeds, eig=jacobi_eig, cache=None):
    """One frame of msl_lines_3d (cache: a dict that keeps the per-keyline results, which do not depend on order or flags, between calls).  line_ends (n, 4) float32, depth (H, W) float32, flags (n,) uint8 or None, Tcw (3, 4) float32, seeds (n,).
    Returns dict(line_depth (n, 2) f32, line_xyz (n, 6) f64, line_ok, line_new, n_support, n_new, lines: the per-keyline results or None)."""
    n = len(line_ends)
    flags = np.zeros(n, np.uint8) if flags is None else np.asarray(flags, np.uint8)
    ld = np.zeros((n, 2), F32); xyz = np.zeros((n, 6), F64); ok = np.zeros(n, np.uint8); sup = np.zeros(n, np.int32)
    lines = [None] * n
    cache = {} if cache is None else cache
    for i in range(n):
        sx, sy, ex, ey = line_ends[i]
        ld[i] = end_depth(depth, sx, sy), end_depth(depth, ex, ey)
    cand = [i for i in range(n) if ld[i, 0] > 0 and ld[i, 1] > 0 and (order == ALL or (int(flags[i]) & 3) != 3)]
    todo = [i for i in cand if i not in cache]
    smp = {i: sample_points(line_ends[i], depth, prm) for i in todo}
    if todo:                                                             # compPt3dCov of every sample of the frame: independent per sample
        DU = du_of(cov0_of(np.concatenate([smp[i][1] for i in todo]), F32(prm["fx"])), eig)
        at = 0
        for i in todo:
            k = len(smp[i][1])
            cache[i] = obtain_3d_line(line_ends[i], depth, Tcw, int(seeds[i]), prm, eig, smp[i] + (DU[at:at + k],))
            at += k
    for i in cand:
        lines[i] = r = cache[i]
        ok[i], xyz[i], sup[i] = r["ok"], r["xyz"], r["n_support"]
    new = select(order, ld, flags, ok, int(prm["max_new_lines"]))
    return dict(line_depth=ld, line_xyz=xyz, line_ok=ok, line_new=new, n_support=sup, n_new=int(new.sum()), lines=lines)

"""A literal, sequential CPU model of Tracking::DetectManhattan (reference src/Tracking.cc:651-844) with
Map::Get[Partial]ManhattanObservation (src/Map.cc:32-123, keys compared as unordered sets), the parity reference of
msl_manhattan_detect[_batch].

Test infrastructure only.  Types as the reference has them: the angles are float dot products evaluated left to right, the scores int
sums of point counts, Mat::cross a float product, cv::determinant of a 3x3 CV_32F matrix in double, cv::SVD in float (LAPACK's sgesdd
here: the device computes the same polar factor U * Vt in double, so Rcw is compared with a tolerance), the products cv::gemm's float
kernel (double accumulation, one rounding per element).  A frame is a dict of manhattanslam_amd.plane; only slot 0 of plane_match is read.

first_maximum is an independent formulation of the choice (every candidate scored, then the first one with the largest score > 0) used
only to cross-check the literal loop.  candidates_fast is the same loop with the table scan replaced by a dictionary built once per frame
and the dot products taken from one float Gram matrix (the same left-to-right expression): tests/test_plane_model.py asserts it equal to
the literal one; it exists because _lookup's scan is unusable on a 65536-row table.  polar64 is the polar factor by a float64 SVD, the
tight reference of the device's double Newton iteration."""
import numpy as np

F32 = np.float32


def _lookup(table, w, keys):
    """The entry of a table whose first w ints are the key set `keys` (unordered), or None."""
    want = sorted(int(k) for k in keys)
    for e in np.asarray(table, np.int32).reshape(-1, w + 1 + w):
        if sorted(int(x) for x in e[:w]) == want:
            return e
    return None


def _index_in_kf(e, w, m):
    """MapPlane::GetIndexInKeyFrame(pKF) of map plane m as the entry records it."""
    for q in range(w):
        if e[q] == m:
            return int(e[w + 1 + q])
    return -1


def _kf_counts(fr, kf, idx, caps):
    """The keyframe point counts of an entry's planes, or None when the entry is no candidate: an index -1 (:713 / :752), and -- as
    include/msl.h defines the flattened tables -- an index outside [0, pcap) or a keyframe slot outside [0, kcap).  caps = (pcap, kcap);
    by default the frame's own extents (its keyframes, and the planes keyframe kf records).  Counts beyond a keyframe's planes are 0."""
    kcap = len(fr["kf_Rwc"]) if caps is None else caps[1]
    if kf < 0 or kf >= kcap:
        return None
    kn = fr["kf_npts"][kf] if kf < len(fr["kf_npts"]) else ()
    pcap = len(kn) if caps is None else caps[0]
    if any(q < 0 or q >= pcap for q in idx):
        return None
    return [int(kn[q]) if q < len(kn) else 0 for q in idx]


def _held(fr, i):
    m = int(np.asarray(fr["plane_match"]).reshape(-1, 3)[i, 0])
    if m < 0 or m >= len(fr["mp_w"]) or not (fr["mp_flags"][m] & 1):
        return None
    return m


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def candidates(fr, mf_ver_th, caps=None):
    """Every candidate of the loop in order: (i, j, k or -1, entry, score, kf, idx) with score > 0 or not."""
    th = F32(mf_ver_th)
    coef = np.asarray(fr["plane_coef"], F32).reshape(-1, 4)
    npts = np.asarray(fr["plane_npts"])
    n = len(coef)
    out = []
    for i in range(n):                                                      # :658
        m1 = _held(fr, i)
        if m1 is None:                                                      # :662-664
            continue
        for j in range(i + 1, n):                                           # :666
            m2 = _held(fr, j)
            if m2 is None:                                                  # :670-672
                continue
            angle12 = _dot(coef[i], coef[j])                                # :674-676
            if angle12 > th or angle12 < -th:                               # :678-680
                continue
            for k in range(j + 1, n):                                       # :682
                m3 = _held(fr, k)
                if m3 is None:
                    continue
                angle13 = _dot(coef[i], coef[k])
                angle23 = _dot(coef[j], coef[k])
                if angle13 > th or angle13 < -th or angle23 > th or angle23 < -th:   # :698-700
                    continue
                e = _lookup(fr["full"], 3, (m1, m2, m3))                    # :702
                if e is None:
                    continue
                kf = int(e[3])
                idx = [_index_in_kf(e, 3, m) for m in (m1, m2, m3)]
                kn = _kf_counts(fr, kf, idx, caps)                          # :712-714
                if kn is None:
                    continue
                score = kn[0] + kn[1] + kn[2] + int(npts[i]) + int(npts[j]) + int(npts[k])
                out.append((i, j, k, e, score, kf, idx))
            e = _lookup(fr["part"], 2, (m1, m2))                            # :741
            if e is None:
                continue
            kf = int(e[2])
            idx = [_index_in_kf(e, 2, m) for m in (m1, m2)]
            kn = _kf_counts(fr, kf, idx, caps)                              # :750-752
            if kn is None:
                continue
            score = kn[0] + kn[1] + int(npts[i]) + int(npts[j])
            out.append((i, j, -1, e, score, kf, idx))
    return out


def _table_dict(table, w):
    """Sorted key tuple -> the first entry holding that key set (what _lookup's scan returns)."""
    d = {}
    for e in np.asarray(table, np.int32).reshape(-1, w + 1 + w):
        d.setdefault(tuple(sorted(e[:w].tolist())), e)
    return d


def candidates_fast(fr, mf_ver_th, caps=None):
    """candidates() with a dictionary lookup, the held planes and the dot products computed once."""
    th = F32(mf_ver_th)
    coef = np.asarray(fr["plane_coef"], F32).reshape(-1, 4)
    npts = [int(x) for x in np.asarray(fr["plane_npts"])]
    n = len(coef)
    held = [_held(fr, i) for i in range(n)]
    a, b = coef[:, None, :], coef[None, :, :]
    G = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    ok = ~((G > th) | (G < -th))                                            # the literal gate: NaN passes
    full, part = _table_dict(fr["full"], 3), _table_dict(fr["part"], 2)
    out = []
    for i in range(n):
        m1 = held[i]
        if m1 is None:
            continue
        for j in range(i + 1, n):
            m2 = held[j]
            if m2 is None or not ok[i, j]:
                continue
            for k in range(j + 1, n):
                m3 = held[k]
                if m3 is None or not ok[i, k] or not ok[j, k]:
                    continue
                e = full.get(tuple(sorted((m1, m2, m3))))
                if e is None:
                    continue
                kf = int(e[3])
                idx = [_index_in_kf(e, 3, m) for m in (m1, m2, m3)]
                kn = _kf_counts(fr, kf, idx, caps)
                if kn is None:
                    continue
                out.append((i, j, k, e, kn[0] + kn[1] + kn[2] + npts[i] + npts[j] + npts[k], kf, idx))
            e = part.get(tuple(sorted((m1, m2))))
            if e is None:
                continue
            kf = int(e[2])
            idx = [_index_in_kf(e, 2, m) for m in (m1, m2)]
            kn = _kf_counts(fr, kf, idx, caps)
            if kn is None:
                continue
            out.append((i, j, -1, e, kn[0] + kn[1] + npts[i] + npts[j], kf, idx))
    return out


def detect_manhattan(fr, mf_ver_th, rcw_in=None, caps=None, fast=False, polar_fn=None):
    """(found, full, Rcw (9,) f32, choice (i, j, k, entry-as-array, score, kf, idx) or None).  Rcw is rcw_in (default zeros) when not
    found.  fast: candidates_fast in place of candidates; polar_fn: polar (default) or polar64."""
    best, maxScore, full = None, 0, False
    for cand in (candidates_fast if fast else candidates)(fr, mf_ver_th, caps):                                  # the literal "score > maxScore" of :718 / :758
        if cand[4] > maxScore:
            maxScore = cand[4]
            best = cand
            full = cand[2] >= 0
    R0 = np.zeros(9, F32) if rcw_in is None else np.array(rcw_in, F32).reshape(9)
    if best is None:                                                        # :778-780
        return 0, 0, R0, None
    return 1, int(full), rotation(fr, best, polar_fn or polar), best


def first_maximum(fr, mf_ver_th, caps=None, fast=False):
    """The choice as the first candidate in loop order that reaches the largest score, when that score is > 0."""
    c = (candidates_fast if fast else candidates)(fr, mf_ver_th, caps)
    if not c or max(x[4] for x in c) <= 0:
        return None
    top = max(x[4] for x in c)
    return next(x for x in c if x[4] == top)


def gemm33(A, B):
    """cv::gemm of two 3x3 CV_32F matrices: double accumulation, one rounding per element."""
    A = np.asarray(A, F32); B = np.asarray(B, F32)
    C = np.zeros((3, 3), F32)
    for r in range(3):
        for c in range(3):
            s = 0.0
            for k in range(3):
                s += float(A[r, k]) * float(B[k, c])
            C[r, c] = F32(s)
    return C


def det3(m):
    """cv::determinant of a 3x3 CV_32F matrix (double)."""
    m = [[float(x) for x in row] for row in np.asarray(m, F32)]
    return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
            m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))


def cross(a, b):
    """cv::Mat::cross of two CV_32F 3-vectors (float)."""
    a = np.asarray(a, F32); b = np.asarray(b, F32)
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F32)


def polar(M):
    """cv::SVD::compute(M, W, U, VT); M = U * VT, in float."""
    U, _, Vt = np.linalg.svd(np.asarray(M, F32))
    return gemm33(U.astype(F32), Vt.astype(F32))


def polar64(M):
    """The same polar factor from a float64 SVD of the same float matrix, U * Vt rounded to float once."""
    U, _, Vt = np.linalg.svd(np.asarray(M, F32).astype(np.float64))
    return (U @ Vt).astype(F32)


def frames_of(fr, cand):
    """MFc, MFm (3x3 f32, columns = the plane normals) before the polar step, with the partial case's cross product and flip."""
    i, j, k, e, _, kf, idx = cand
    coef = np.asarray(fr["plane_coef"], F32).reshape(-1, 4)
    kc = np.asarray(fr["kf_coef"][kf], F32).reshape(-1, 4)
    full = k >= 0
    c1, c2 = coef[i, :3], coef[j, :3]
    m1, m2 = kc[idx[0], :3], kc[idx[1], :3]
    if full:
        c3, m3 = coef[k, :3], kc[idx[2], :3]
    else:                                                                   # :760-770
        c3, m3 = cross(c1, c2), cross(m1, m2)
    MFc = np.stack([c1, c2, c3], 1).astype(F32)                             # :776-784
    MFm = np.stack([m1, m2, m3], 1).astype(F32)
    if not full and abs(det3(MFc) + 1) < 0.5:                               # :786-790
        MFc[:, 2] = -c3
    if not full and abs(det3(MFm) + 1) < 0.5:                               # :808-812
        MFm[:, 2] = -m3
    return MFc, MFm


def rotation(fr, cand, polar_fn=polar):
    """manhattanRcw (9,) f32 of a chosen candidate (:772-840)."""
    MFc, MFm = frames_of(fr, cand)
    MFc, MFm = polar_fn(MFc), polar_fn(MFm)                                       # :792-796, :814-818
    kR = np.asarray(fr["kf_Rwc"][cand[5]], F32).reshape(3, 3)
    Rwc = gemm33(gemm33(kR, MFm), MFc.T)                                    # :820
    return np.ascontiguousarray(Rwc.T).reshape(9)                           # :821

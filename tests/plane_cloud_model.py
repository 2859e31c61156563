"""Sequential model of msl_plane_clouds and msl_map_plane_merge: the tail of Frame::ExtractPlanes (reference src/Frame.cc:611-653 with
Frame::MaxPointDistanceFromPlane, :662-709) and MapPlane::UpdateCoefficientsAndPoints(Frame&, id) (src/MapPlane.cc:201-218) as the loop of
src/Tracking.cc:429-436 calls it.  This file is the contract: the kernels of msl_plane_cloud.hip give its bytes.  NumPy
float32 / float64 / int64 element-wise arithmetic only (+ - * / sqrt, floor, rint), which rounds exactly as the device's scalar operations do.
The pins against PCL:
  * pcl::VoxelGrid: voxel = floorf(x * (1.0f / leaf)) per axis, output voxels in ascending (vz, vy, vx); a point that is not finite or has a
    |coordinate| >= 32768 is skipped; the centroid of a voxel is the mean of the coordinates quantised to 2^-24 m, summed as integers (no order);
    colour: integer sums, a float quotient, truncated; a bounding box of more than INT32_MAX cells and more than MAX_VOXELS voxels are statuses
  * pcl::transformPointCloud: (float)(T[4r] x + T[4r + 1] y + T[4r + 2] z + T[4r + 3]) in double, left to right
  * pcl::SACSegmentation: the project's counter-based sampler (tests/pnp_model.py: hash32) seeded with seed ^ fmix32(detector plane), three
    distinct points by swap-with-back; a sample with a zero cross product uses up its iteration; strict `count > best`; the stop
    q^it <= 1 - probability by repeated multiplication; the refit is the eigenvector of the smallest eigenvalue of the centred scatter matrix
    (tests/pnp_model.py: jacobi_eig), sums in 256 interleaved partials and a pairwise tree."""
import numpy as np

from tests.pnp_model import _fmix, hash32, jacobi_eig

F32, F64 = np.float32, np.float64
MAX_VOXELS = 4096                # MSL_PLANE_CLOUD_MAX_VOXELS
FAR = 32768.0
BIAS = 1 << 20                   # voxel indices lie in [-2^20, 2^20): leaf >= 1 / 32
LANES = 256                      # partial sums of the refit

KEPT, GATE, FEW, NO_MODEL, VOXELS, GRID, NO_ROOM = range(7)           # msl_plane_clouds: status
UNTOUCHED, MERGED = 0, 1                                             # msl_map_plane_merge: merge_status (failures: VOXELS, GRID, NO_ROOM)


def params(leaf=0.2, dis_th=0.05, max_iterations=50, probability=0.99):
    return dict(leaf=leaf, dis_th=dis_th, max_iterations=max_iterations, probability=probability)


# ---- voxel grid -----------------------------------------------------------------------------------------------------------------------------
def quantise(x):
    """(int64)rint((double)x * 2^24) of float32 values."""
    return np.rint(np.asarray(x, F32).astype(F64) * 16777216.0).astype(np.int64)


def voxel_of(pts, leaf):
    """(n, 3) int64 voxel indices of float32 points."""
    inv = F32(1.0) / F32(leaf)
    return np.floor(np.asarray(pts, F32) * inv).astype(np.int64)


def usable(pts):
    pts = np.asarray(pts, F32).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        return np.all(np.isfinite(pts), axis=1) & np.all(np.abs(pts) < F32(FAR), axis=1)


def voxel_grid(pts, rgb, leaf):
    """pcl::VoxelGrid of a cloud.  pts (n, 3) float32, rgb (n, 3) uint8 or None.  Returns (status, pts_out (m, 3) f32, rgb_out (m, 3) u8 or
    None); status 0, VOXELS or GRID (outputs empty then)."""
    pts = np.asarray(pts, F32).reshape(-1, 3)
    empty = (np.zeros((0, 3), F32), None if rgb is None else np.zeros((0, 3), np.uint8))
    keep = usable(pts)
    pts = pts[keep]
    if rgb is not None:
        rgb = np.asarray(rgb, np.uint8).reshape(-1, 3)[keep]
    if len(pts) == 0:
        return 0, *empty
    v = voxel_of(pts, leaf)
    span = v.max(axis=0) - v.min(axis=0) + 1
    if int(span[0]) * int(span[1]) * int(span[2]) > 2147483647:
        return GRID, *empty
    key = ((v[:, 2] + BIAS) << 42) | ((v[:, 1] + BIAS) << 21) | (v[:, 0] + BIAS)
    uniq, inverse = np.unique(key, return_inverse=True)
    if len(uniq) > MAX_VOXELS:
        return VOXELS, *empty
    q = quantise(pts)
    sums = np.zeros((len(uniq), 3), np.int64)
    np.add.at(sums, inverse, q)
    cnt = np.bincount(inverse, minlength=len(uniq)).astype(np.int64)
    out = (sums.astype(F64) / 16777216.0 / cnt.astype(F64)[:, None]).astype(F32)
    crgb = None
    if rgb is not None:
        cs = np.zeros((len(uniq), 3), np.int64)
        np.add.at(cs, inverse, rgb.astype(np.int64))
        crgb = (cs.astype(np.uint32).astype(F32) / cnt.astype(np.uint32).astype(F32)[:, None]).astype(np.uint8)
    return 0, out, crgb


# ---- gate -----------------------------------------------------------------------------------------------------------------------------------
def detector_coef(normal, center):
    """(a, b, c, d) float32 of a detector plane (src/Frame.cc:626-643)."""
    n = np.asarray(normal, F64); c = np.asarray(center, F64)
    d = -(n[0] * c[0] + n[1] * c[1] + n[2] * c[2])
    return np.array([n[0], n[1], n[2], d]).astype(F32)


def distances(coef, pts):
    """float32 |a x + b y + c z + d|, left to right."""
    coef = np.asarray(coef, F32); pts = np.asarray(pts, F32).reshape(-1, 3)
    return np.abs(coef[0] * pts[:, 0] + coef[1] * pts[:, 1] + coef[2] * pts[:, 2] + coef[3])


# ---- RANSAC ---------------------------------------------------------------------------------------------------------------------------------
def plane_seed(seed, plane):
    return int(np.uint64(int(seed) & 0xFFFFFFFF) ^ _fmix(np.uint64(plane)))


def sample3(seed, k, N):
    avail = list(range(N))
    out = []
    for j in range(3):
        r = (int(hash32(seed, k, j)) * len(avail)) >> 32
        out.append(avail[r])
        avail[r] = avail[-1]
        avail.pop()
    return out


def plane_of(p0, p1, p2):
    """The float32 plane of three points, or None when the cross product has no norm."""
    a = p1 - p0; b = p2 - p0
    c = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F32)
    nn = np.sqrt(F32(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]))
    if not nn > 0:
        return None
    n = c / nn
    d = -(n[0] * p0[0] + n[1] * p0[1] + n[2] * p0[2])
    return np.array([n[0], n[1], n[2], d], F32)


def stop_after(it, count, N, probability, max_iterations):
    """The stop test after `it` iterations with a best count of `count` among N points."""
    if it >= max_iterations:
        return True
    w = F64(count) / F64(N)
    q = F64(1.0) - w * w * w
    p = F64(1.0)
    for _ in range(it):
        p = p * q
    return bool(p <= F64(1.0) - F64(probability))


def tree_sum(values):
    """Sum of float64 values (n, ...) in the fixed layout: element i to partial i mod 256 in ascending order, then a pairwise tree."""
    values = np.asarray(values, F64)
    part = np.zeros((LANES,) + values.shape[1:], F64)
    for i0 in range(0, len(values), LANES):
        chunk = values[i0:i0 + LANES]
        part[:len(chunk)] = part[:len(chunk)] + chunk
    h = LANES // 2
    while h >= 1:
        part = part[:h] + part[h:2 * h]
        h //= 2
    return part[0]


def refit(pts):
    """(a, b, c, d) float32 of the least-squares plane of float32 points (more than 3)."""
    P = np.asarray(pts, F32).astype(F64)
    cen = tree_sum(P) / F64(len(P))
    D = P - cen
    prod = np.stack([D[:, 0] * D[:, 0], D[:, 0] * D[:, 1], D[:, 0] * D[:, 2], D[:, 1] * D[:, 1], D[:, 1] * D[:, 2], D[:, 2] * D[:, 2]], axis=1)
    s = tree_sum(prod)
    A = np.array([[s[0], s[1], s[2]], [s[1], s[3], s[4]], [s[2], s[4], s[5]]], F64)
    _, ut = jacobi_eig(A)
    v = ut[2]                                                                  # the smallest eigenvalue, the highest index on ties
    nn = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    n = v / nn
    d = -(n[0] * cen[0] + n[1] * cen[1] + n[2] * cen[2])
    return np.array([n[0], n[1], n[2], d]).astype(F32)


def ransac(pts, seed, prm, trace=None):
    """SACSegmentation on the coarse cloud (N >= 4).  Returns the float32 coefficients or None (no hypothesis at all)."""
    pts = np.asarray(pts, F32).reshape(-1, 3)
    N = len(pts)
    th = F32(prm["dis_th"])
    best, best_n, best_in = None, 0, None
    it = 0
    while True:
        s = sample3(seed, it, N)
        it += 1
        h = plane_of(pts[s[0]], pts[s[1]], pts[s[2]])
        if h is not None:
            with np.errstate(invalid="ignore"):
                dist = distances(h, pts)
                inl = dist < th
            if trace is not None:                                              # how close a decision comes to its threshold
                trace["margin"] = min(trace.get("margin", np.inf), float(np.min(np.abs(dist.astype(F64) - F64(th)))))
            if int(inl.sum()) > best_n:
                best, best_n, best_in = h, int(inl.sum()), inl
        if stop_after(it, best_n, N, prm["probability"], prm["max_iterations"]):
            break
    if trace is not None:
        trace.update(iterations=it, count=best_n, hypothesis=best, inliers=best_in)
    if best is None:
        return None
    return refit(pts[best_in]) if best_n > 3 else best


# ---- msl_plane_clouds -----------------------------------------------------------------------------------------------------------------------
def plane_cloud(cloud, rgb, indices, normal, center, seed, plane, prm, trace=None):
    """One detector plane: (status, coef (4,) f32, pts (m, 3) f32, rgb (m, 3) u8 or None).  indices outside the cloud are absent."""
    cloud = np.asarray(cloud, F64).reshape(-1, 3)
    idx = np.asarray(indices, np.int64)
    idx = idx[(idx >= 0) & (idx < len(cloud))]
    st, pts, crgb = voxel_grid(cloud[idx].astype(F32), None if rgb is None else np.asarray(rgb, np.uint8).reshape(-1, 3)[idx], prm["leaf"])
    if st:
        return st, None, pts, crgb
    coef = detector_coef(normal, center)
    with np.errstate(invalid="ignore"):
        dist = distances(coef, pts)
        if trace is not None and len(dist):
            trace["margin"] = min(trace.get("margin", np.inf), float(np.min(np.abs(dist.astype(F64) - F64(F32(prm["dis_th"]))))))
        if np.any(dist > F32(prm["dis_th"])):
            return GATE, None, pts, crgb
    if len(pts) < 4:
        return FEW, None, pts, crgb
    new = ransac(pts, plane_seed(seed, plane), prm, trace)
    if new is None:
        return NO_MODEL, None, pts, crgb
    old = coef[3]
    if (new[3] < 0 and old > 0) or (new[3] > 0 and old < 0):
        new = -new
    return KEPT, new, pts, crgb


def plane_clouds(fr, prm, pcap, ptcap):
    """One frame: dict cloud (V, 3) f64, rgb (V, 3) u8 or None, vertices: list of index arrays, planes: list of (normal, center), seed.
    Returns dict n_out, plane_coef (n, 4), plane_npts (n,), plane_src (n,), pt_off (n + 1,), pts, rgb, status (len(planes),)."""
    status = np.zeros(len(fr["planes"]), np.int32)
    coef, npts, src, off, pts, cols = [], [], [], [0], [], []
    full = False
    for i, (normal, center) in enumerate(fr["planes"]):
        st, c, p, col = plane_cloud(fr["cloud"], fr.get("rgb"), fr["vertices"][i], normal, center, fr["seed"], i, prm)
        if st == KEPT:
            if full or len(coef) == pcap or off[-1] + len(p) > ptcap:
                full = True
                st = NO_ROOM
            else:
                coef.append(c); npts.append(len(p)); src.append(i); off.append(off[-1] + len(p)); pts.append(p); cols.append(col)
        status[i] = st
    has_rgb = fr.get("rgb") is not None
    return dict(n_out=len(coef), plane_coef=np.array(coef, F32).reshape(-1, 4), plane_npts=np.array(npts, np.int32), plane_src=np.array(src, np.int32),
                pt_off=np.array(off, np.int32), pts=np.concatenate(pts).reshape(-1, 3) if pts else np.zeros((0, 3), F32),
                rgb=(np.concatenate(cols).reshape(-1, 3) if cols else np.zeros((0, 3), np.uint8)) if has_rgb else None, status=status)


# ---- msl_map_plane_merge --------------------------------------------------------------------------------------------------------------------
def transform(Twc, pts):
    """float32 points through the 12 doubles of Twc (row-major rows 0-2)."""
    T = np.asarray(Twc, F64).reshape(3, 4)
    P = np.asarray(pts, F32).astype(F64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return np.stack([T[r, 0] * P[:, 0] + T[r, 1] * P[:, 1] + T[r, 2] * P[:, 2] + T[r, 3] for r in range(3)], axis=1).astype(F32)


def map_plane_merge(fr, prm, ptcap):
    """One frame: dict clouds: list of (m, 3) f32 frame-plane clouds, rgbs: list or None, merge_into: list of rows or -1, Twc (12,) f64,
    mp_clouds: list of (n, 3) f32, mp_rgbs: list or None.  Returns dict clouds, rgbs (the new map), pt_off, status (len(mp_clouds),)."""
    n_map = len(fr["mp_clouds"])
    has_rgb = fr.get("mp_rgbs") is not None
    clouds = [np.asarray(c, F32).reshape(-1, 3) for c in fr["mp_clouds"]]
    rgbs = [np.asarray(c, np.uint8).reshape(-1, 3) for c in fr["mp_rgbs"]] if has_rgb else [None] * n_map
    status = np.zeros(n_map, np.int32)
    failed = np.zeros(n_map, bool)
    for k, j in enumerate(fr["merge_into"]):
        if j < 0 or j >= n_map:
            continue
        both = np.concatenate([transform(fr["Twc"], fr["clouds"][k]), clouds[j]])
        col = np.concatenate([np.asarray(fr["rgbs"][k], np.uint8).reshape(-1, 3), rgbs[j]]) if has_rgb else None
        st, p, c = voxel_grid(both, col, prm["leaf"])
        if st:                                                                 # the row keeps its cloud; the first failure is its status
            if not failed[j]:
                status[j] = st
                failed[j] = True
        else:
            clouds[j], rgbs[j] = p, c
            if not failed[j]:
                status[j] = MERGED
    off = [0]
    full = False
    for j in range(n_map):
        if full or off[-1] + len(clouds[j]) > ptcap:
            full = True
            status[j] = NO_ROOM
            clouds[j] = np.zeros((0, 3), F32)
            rgbs[j] = np.zeros((0, 3), np.uint8) if has_rgb else None
        off.append(off[-1] + len(clouds[j]))
    return dict(clouds=clouds, rgbs=rgbs if has_rgb else None, pt_off=np.array(off, np.int32), status=status)

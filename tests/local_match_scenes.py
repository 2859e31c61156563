"""Inputs for the local-map matching tests (Tracking::SearchLocalPoints): hand-made frames for the model's first-principles tests and
random ragged scenes for the GPU parity tests.  Per-frame dicts as manhattanslam_amd.match.pack_local_points takes them."""
import math

import numpy as np

from tests import match_scenes as ms

KEYPOINT_DTYPE = ms.KEYPOINT_DTYPE
LOG_SCALE = np.float32(math.log(1.2))          # Frame::mfLogScaleFactor = log(mfScaleFactor), a float


def params(th=3.0, w=640, h=480, fx=517.3, fy=516.5, cx=318.6, cy=255.3, bf=40.0, view_cos_limit=0.5, nn_ratio=0.8, nlevels=8, scale=1.2):
    from manhattanslam_amd import LOCAL_MATCH_PARAMS_DTYPE
    p = ms.params(None, th, False, w=w, h=h, fx=fx, fy=fy, cx=cx, cy=cy, bf=bf, dtype=LOCAL_MATCH_PARAMS_DTYPE, nlevels=nlevels, scale=scale)
    p["log_scale_factor"], p["view_cos_limit"], p["nn_ratio"] = np.float32(math.log(scale)), view_cos_limit, nn_ratio
    return p


def desc_at(d):
    """A descriptor at Hamming distance d from the all-zero one."""
    out = np.zeros(32, np.uint8)
    bits = np.zeros(256, np.uint8)
    bits[:d] = 1
    out[:] = np.packbits(bits)
    return out


def frame(p, kps):
    """kps: list of (x, y, octave, hamming distance to the zero descriptor, uright, flags)."""
    n = len(kps)
    k = np.zeros(n, KEYPOINT_DTYPE)
    xy = np.array([[a[0], a[1]] for a in kps], np.float32).reshape(n, 2)
    k["x"], k["y"] = xy[:, 0], xy[:, 1]
    k["octave"] = [a[2] for a in kps]
    k["class_id"] = -1
    return dict(kps=k, un_xy=xy, uright=np.array([a[4] for a in kps], np.float32), grid_cell=ms.grid_cells(xy, p),
                desc=np.stack([desc_at(a[3]) for a in kps]) if n else np.zeros((0, 32), np.uint8),
                flags=np.array([a[5] for a in kps], np.uint8))


def points(pts):
    """pts: list of (xyz, normal, (mfMinDistance, mfMaxDistance), flags); every point has the all-zero descriptor."""
    m = len(pts)
    return dict(xyz=np.array([a[0] for a in pts], np.float32).reshape(m, 3), normal=np.array([a[1] for a in pts], np.float32).reshape(m, 3),
                dist=np.array([a[2] for a in pts], np.float32).reshape(m, 2), desc=np.zeros((m, 32), np.uint8),
                flags=np.array([a[3] for a in pts], np.uint8))


def rotation(rng, deg):
    a = rng.normal(size=3)
    a *= math.radians(deg) / np.linalg.norm(a)
    th = np.linalg.norm(a)
    k = a / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K


def random_frame(seed, p, n_cur=1000, n_local=4000, preheld=0.3, cluster=False, conflict=False, desc_noise=10):
    """A current frame of n_cur keypoints and n_local local map points under a random pose.  Most points project next to a keypoint
    whose octave is near the point's predicted level and whose descriptor is a noisy copy of the point's; the rest are unrelated,
    behind the camera, out of the image, out of their distance range or seen too obliquely.  cluster: everything in a small region
    (dozens of candidates per window, more than the 32 stored); conflict: many points share a few keypoints (many fixpoint rounds)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    fx, fy, cx, cy, bf = (float(p[k][0]) for k in ("fx", "fy", "cx", "cy", "bf"))
    W, H = float(p["maxX"][0]), float(p["maxY"][0])
    nlevels, scale = int(p["nlevels"][0]), ms.level_scale(p)
    R = rotation(rng, 8.0)
    t = rng.normal(0, 0.3, 3)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = R, t
    T64 = T.astype(np.float64)
    Rwc, Ow = T64[:3, :3].T, -T64[:3, :3].T @ T64[:3, 3]
    if cluster:
        xy = np.stack([rng.uniform(250, 330, n_cur), rng.uniform(180, 240, n_cur)], 1)
    else:
        xy = np.stack([rng.uniform(2, W - 2, n_cur), rng.uniform(2, H - 2, n_cur)], 1)
    xy = np.round(xy * 4).astype(np.float32) / 4
    depth = rng.uniform(0.8, 6.0, n_cur)
    kps = np.zeros(n_cur, KEYPOINT_DTYPE)
    kps["x"], kps["y"] = xy[:, 0], xy[:, 1]
    kps["octave"] = rng.integers(0, nlevels, n_cur)
    kps["class_id"] = -1
    desc = rng.integers(0, 256, (n_cur, 32), dtype=np.uint8)
    if conflict:   # a handful of distinct descriptors: every point's best is one of few keypoints
        desc = desc[rng.integers(0, 6, n_cur)]
    uright = np.where(rng.random(n_cur) < 0.8, xy[:, 0] - bf / depth, -1.0).astype(np.float32)
    u = rng.random(n_cur)
    cflags = np.where(u < preheld / 2, 3, np.where(u < preheld, 1, 0)).astype(np.uint8)
    cur = dict(kps=kps, un_xy=xy, uright=uright, grid_cell=ms.grid_cells(xy, p), desc=desc, flags=cflags)
    # local points: back-projections of keypoints (plus noise) through the pose
    src = rng.integers(0, min(n_cur, 40) if conflict else n_cur, n_local) if n_cur else np.zeros(n_local, np.int64)
    if n_cur:
        uu = xy[src, 0] + rng.normal(0, 1.0, n_local); vv = xy[src, 1] + rng.normal(0, 1.0, n_local); zz = depth[src] * rng.uniform(0.97, 1.03, n_local)
    else:
        uu = rng.uniform(0, W, n_local); vv = rng.uniform(0, H, n_local); zz = rng.uniform(1, 5, n_local)
    Pc = np.stack([(uu - cx) * zz / fx, (vv - cy) * zz / fy, zz], 1)
    kind = rng.random(n_local)
    Pc[kind < 0.02, 2] *= -1                                             # behind the camera
    Pc[(kind >= 0.02) & (kind < 0.04), 0] += zz[(kind >= 0.02) & (kind < 0.04)] * 2.0   # out of the image
    Pw = (Rwc @ Pc.T).T + Ow
    PO = Pw - Ow
    dist = np.linalg.norm(PO, axis=1)
    # normal: the viewing direction tilted by 0..75 degrees (cos below 0.5 for the most tilted), some exactly along it (cos > 0.998)
    dirn = PO / dist[:, None]
    tilt = np.radians(np.where(rng.random(n_local) < 0.2, rng.uniform(0, 2.5, n_local), rng.uniform(0, 75, n_local)))
    perp = np.cross(dirn, rng.normal(size=(n_local, 3)))
    perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    normal = dirn * np.cos(tilt)[:, None] + perp * np.sin(tilt)[:, None]
    # distance range: a level near the keypoint's octave: mfMaxDistance = dist * scale^level (+ jitter),
    # mfMinDistance = mfMaxDistance / scale^(nlevels - 1)
    lvl = np.clip(kps["octave"][src] + rng.integers(0, 2, n_local), 0, nlevels - 1) if n_cur else rng.integers(0, nlevels, n_local)
    dmax = dist * scale ** (lvl - rng.uniform(0.05, 0.95, n_local))
    dmin = dmax / scale ** (nlevels - 1)
    out_range = (kind >= 0.04) & (kind < 0.06)
    dmax[out_range] = dist[out_range] / 1.3                               # beyond 1.2 * mfMaxDistance
    mdesc = desc[src].copy() if n_cur else rng.integers(0, 256, (n_local, 32), dtype=np.uint8)
    flip = rng.integers(0, 256, (n_local, desc_noise))
    for k in range(desc_noise):
        mdesc[np.arange(n_local), flip[:, k] // 8] ^= (1 << (flip[:, k] % 8)).astype(np.uint8)
    unrelated = rng.random(n_local) < 0.1
    mdesc[unrelated] = rng.integers(0, 256, (int(unrelated.sum()), 32), dtype=np.uint8)
    mflags = ((rng.random(n_local) < 0.9).astype(np.uint8)) | ((rng.random(n_local) < 0.7).astype(np.uint8) << 1)
    local = dict(xyz=Pw.astype(np.float32), normal=normal.astype(np.float32), dist=np.stack([dmin, dmax], 1).astype(np.float32), desc=mdesc,
                 flags=mflags)
    return cur, local, T


def empty_local(local):
    return {k: v[:0] for k, v in local.items()}

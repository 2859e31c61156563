"""Seeded synthetic inputs for the map-line matching tests (LSDmatcher::SearchByProjection, both overloads): 3-D lines projected to keylines
with pixel noise, LBD-sized (32-byte) descriptors at controlled Hamming distances, octaves 0-3 (0 .. octaves - 1), near-vertical lines (x1 == x2), lines behind
the camera, lines at the ends of their distance window (predicted level -1, nlevels, nlevels + 1), many lines on a few keylines, pre-held
keylines with and without observations, and same-level / different-level ties.  Per-frame dicts as manhattanslam_amd.match.pack_lines_last /
pack_local_lines take them."""
import math

import numpy as np

from tests import line_match_model as lmm
from tests import local_match_scenes as ls

F32 = np.float32


def params(th=15.0, view_cos_limit=0.6, nn_ratio=0.6, nlevels=8, scale=1.2):
    """msl_line_match_params for the TUM-like camera of the point tests (640 x 480; by default 8 levels of 1.2)."""
    return ls.params(th, view_cos_limit=view_cos_limit, nn_ratio=nn_ratio, nlevels=nlevels, scale=scale)


def desc_flip(rng, d, nbits):
    """d with nbits distinct bits flipped: at Hamming distance exactly nbits."""
    out = d.copy()
    for b in rng.choice(256, nbits, replace=False):
        out[b // 8] ^= np.uint8(1 << (b % 8))
    return out


def keylines(xy1, xy2, octave, angle):
    from manhattanslam_amd import KEYLINE_DTYPE
    n = len(octave)
    kl = np.zeros(n, KEYLINE_DTYPE)
    kl["x"] = 0.5 * (xy1[:, 0] + xy2[:, 0])
    kl["y"] = 0.5 * (xy1[:, 1] + xy2[:, 1])
    kl["angle"], kl["octave"] = angle, octave
    return kl


def pose(rng, deg=4.0, trans=0.1):
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = ls.rotation(rng, deg), rng.normal(0, trans, 3)
    return T


def _lines_in_camera(rng, n, W=640.0, H=480.0, fx=517.3, fy=516.5, cx=318.6, cy=255.3):
    """n 3-D segments in the camera frame whose endpoints project inside the image: (A, B) (n, 3) each."""
    z = rng.uniform(1.0, 5.0, (n, 2))
    u = rng.uniform(30, W - 30, (n, 2)); v = rng.uniform(30, H - 30, (n, 2))
    A = np.stack([(u[:, 0] - cx) / fx * z[:, 0], (v[:, 0] - cy) / fy * z[:, 0], z[:, 0]], 1)
    B = np.stack([(u[:, 1] - cx) / fx * z[:, 1], (v[:, 1] - cy) / fy * z[:, 1], z[:, 1]], 1)
    return A, B


def _to_world(T, A):
    R, t = T[:3, :3].astype(np.float64), T[:3, 3].astype(np.float64)
    return (A - t) @ R


def _project(p, T, xyz6):
    """(u1, v1, u2, v2) of the model, or None."""
    res = lmm.project_line(p, np.asarray(T, F32)[:3, :4], xyz6)
    return None if res is None else np.array([float(x) for x in res[:4]])


def frame_pair(seed, p, n_kl=40, n_last=40, obs_frac=0.7, flag_frac=0.9, vertical=0, behind=0.05, fwd=0.0, octaves=None, noise=1.0,
               angle_mode="mixed", few=0, T=None):
    """A current frame of n_kl keylines and a last frame of n_last map lines.  Most last-frame lines project (through the current pose) next
    to a keyline whose descriptor is a noisy copy of theirs.  vertical: that many lines with x1 == x2 exactly (identity pose);
    fwd: camera motion along z (positive: forward, negative: backward search mode); few: every line near one of `few` keylines;
    octaves: keyline and last-line octaves are drawn from [0, octaves), by default min(4, nlevels)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    octaves = octaves or min(4, int(lmm._p(p)["nlevels"]))
    T = (np.eye(4, dtype=np.float32) if vertical else pose(rng)) if T is None else np.asarray(T, np.float32)
    Tl = T.copy()
    Tl[2, 3] += F32(fwd)
    A, B = _lines_in_camera(rng, max(n_last, 1))
    if vertical:
        A[:vertical, 0] = 0.25 * A[:vertical, 2]; B[:vertical, 0] = 0.25 * B[:vertical, 2]   # X / Z the same: u1 == u2 exactly
        A[:vertical, 2] = 2.0 ** rng.integers(0, 3, vertical); B[:vertical, 2] = 2.0 ** rng.integers(0, 3, vertical)
        A[:vertical, 0] = 0.25 * A[:vertical, 2]; B[:vertical, 0] = 0.25 * B[:vertical, 2]
    back = rng.random(len(A)) < behind
    A[back, 2] *= -1
    xyz = np.concatenate([_to_world(T, A), _to_world(T, B)], 1)[:n_last]
    base = rng.integers(0, 256, (max(n_last, 1), 32), dtype=np.uint8)[:n_last]
    # keylines: most at a last-frame line's projection (+ noise), the rest random
    proj = [(_project(p, T, xyz[i]), i) for i in range(n_last)]
    proj = [(q, i) for q, i in proj if q is not None and np.all(np.isfinite(q))]
    src = rng.permutation(len(proj))[:n_kl]
    if few:
        src = src[:few]
    xy1 = rng.uniform(20, 620, (n_kl, 2)); xy2 = rng.uniform(20, 620, (n_kl, 2)); xy2[:, 1] = xy2[:, 1] % 460
    desc = rng.integers(0, 256, (n_kl, 32), dtype=np.uint8)
    slope = np.zeros(n_kl)
    for k in range(n_kl):
        if len(src) == 0 or (not few and k >= len(src)):
            break
        q, i = proj[src[k % len(src)]]
        xy1[k] = q[:2] + rng.normal(0, noise, 2); xy2[k] = q[2:] + rng.normal(0, noise, 2)
        desc[k] = desc_flip(rng, base[i], int(rng.integers(0, 60)))
        with np.errstate(divide="ignore", invalid="ignore"):
            slope[k] = (q[1] - q[3]) / (q[0] - q[2]) if q[0] != q[2] else 0.0
    if angle_mode == "slope":
        angle = slope + rng.uniform(-0.05, 0.2, n_kl)
    elif angle_mode == "atan":
        angle = np.arctan2(xy1[:, 1] - xy2[:, 1], xy1[:, 0] - xy2[:, 0])
    else:   # half next to the projected slope (the positive side of the test decides), half LSD-like angles
        angle = np.where(rng.random(n_kl) < 0.5, slope + rng.uniform(-0.05, 0.3, n_kl), np.arctan2(xy1[:, 1] - xy2[:, 1], xy1[:, 0] - xy2[:, 0]))
    cur = dict(kl=keylines(xy1, xy2, rng.integers(0, octaves, n_kl), angle.astype(F32)), desc=desc, ends=np.concatenate([xy1, xy2], 1))
    flags = ((rng.random(n_last) < flag_frac).astype(np.uint8)) | ((rng.random(n_last) < obs_frac).astype(np.uint8) << 1)
    last = dict(xyz=xyz, desc=base, flags=flags, octave=rng.integers(0, octaves, n_last).astype(np.int32))
    return cur, last, T, Tl


def _window_end(p, T, xyz6, level, nlevels):
    """(mfMinDistance, mfMaxDistance) that put the line's predicted level at `level` (-1, nlevels or nlevels + 1), or None."""
    Tm = np.asarray(T, F32)[:3, :4]
    res = lmm.project_line(p, Tm, xyz6)
    if res is None:
        return None
    SP, EP = res[4], res[5]
    OM = (SP * F32(0.5) + EP * F32(0.5) + F32(0)) - lmm.gemm3(Tm, True, -1.0, Tm[:, 3])
    dist = F32(math.sqrt(sum(float(x) * float(x) for x in OM)))
    ls_ = F32(lmm._p(p)["log_scale_factor"])
    if level == -1:   # dist == 1.2f * dmax exactly: search the float dmax next to dist / 1.2
        d0 = F32(float(dist) / 1.2)
        for k in range(-8, 9):
            dmax = np.nextafter(d0, F32(np.inf) if k > 0 else F32(0), dtype=F32) if k else d0
            for _ in range(abs(k) - 1):
                dmax = np.nextafter(dmax, F32(np.inf) if k > 0 else F32(0), dtype=F32)
            if not (dist > F32(1.2) * dmax) and lmm.predict_level(dmax, dist, ls_) == -1:
                return F32(0.0), dmax
        return None
    dmax = F32(float(dist) * ls.ms.level_scale(p) ** (level - 0.5))
    return (F32(0.0), dmax) if lmm.predict_level(dmax, dist, ls_) == level else None


def local_frame(seed, p, n_kl=40, n_local=2000, preheld=0.3, few=0, ends=True, octaves=None, noise=1.0, T=None):
    """A current frame of n_kl keylines and n_local local map lines under a random pose.  Most lines project near a keyline (a noisy copy of
    its descriptor); some are unrelated, behind the camera, outside their distance window, seen too obliquely or exactly head-on (viewCos
    > 0.998 for the 5-pixel radius); with ends, some sit at the distance-window ends (levels -1, nlevels, nlevels + 1).  few: all lines
    around `few` keylines (a deep fixpoint)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    octaves = octaves or min(4, int(lmm._p(p)["nlevels"]))
    T = pose(rng) if T is None else np.asarray(T, np.float32)
    m = max(n_local, 1)
    A, B = _lines_in_camera(rng, m)
    if few:   # every line is a copy of one of `few` segments (+ 1 px): many lines compete for a few keylines
        tA, tB = A[:few].copy(), B[:few].copy()
        pick = rng.integers(0, few, m)
        s = rng.uniform(0.9, 1.1, m)[:, None]
        A = tA[pick] * s + rng.normal(0, 0.002, (m, 3)); B = tB[pick] * s + rng.normal(0, 0.002, (m, 3))
    kind = rng.random(m)
    A[kind < 0.03, 2] *= -1; B[(kind >= 0.03) & (kind < 0.05), 2] *= -1                       # one endpoint behind the camera
    xyz = np.concatenate([_to_world(T, A), _to_world(T, B)], 1)
    Tm = T[:3, :4]
    Ow = -T[:3, :3].astype(np.float64).T @ T[:3, 3].astype(np.float64)
    mid = 0.5 * (xyz[:, :3] + xyz[:, 3:]) - Ow
    dist = np.linalg.norm(mid, axis=1)
    dirn = mid / dist[:, None]
    tilt = np.radians(np.where(rng.random(m) < 0.25, 0.0, rng.uniform(0, 60, m)))   # 0: viewCos ~ 1 (> 0.998)
    perp = np.cross(dirn, rng.normal(size=(m, 3))); perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    normal = dirn * np.cos(tilt)[:, None] + perp * np.sin(tilt)[:, None]
    nlevels, scale = int(lmm._p(p)["nlevels"]), ls.ms.level_scale(p)
    lvl = rng.integers(0, octaves, m) + rng.integers(0, 2, m)
    dmax = dist * scale ** (lvl - rng.uniform(0.05, 0.95, m))
    dmin = dmax / scale ** (nlevels - 1)
    out = (kind >= 0.05) & (kind < 0.07)
    dmax[out] = dist[out] / 1.3
    dd = np.stack([dmin, dmax], 1).astype(F32)
    if ends:
        for j, level in zip(range(0, min(m, 60), 1), [-1, nlevels, nlevels + 1] * 20):
            w = _window_end(p, Tm, xyz[j], level, nlevels)
            if w is not None:
                dd[j] = w
    # keylines
    base = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    proj = [(_project(p, T, xyz[i]), i) for i in range(min(m, 4 * n_kl + 50))]
    proj = [(q, i) for q, i in proj if q is not None and np.all(np.isfinite(q))]
    xy1 = rng.uniform(20, 620, (n_kl, 2)); xy2 = rng.uniform(20, 460, (n_kl, 2))
    kdesc = rng.integers(0, 256, (n_kl, 32), dtype=np.uint8)
    slope = np.zeros(n_kl)
    for k in range(min(n_kl, len(proj))):
        q, i = proj[k]
        xy1[k] = q[:2] + rng.normal(0, noise, 2); xy2[k] = q[2:] + rng.normal(0, noise, 2)
        kdesc[k] = desc_flip(rng, base[i], int(rng.integers(0, 50)))
        slope[k] = (q[1] - q[3]) / (q[0] - q[2]) if q[0] != q[2] else 0.0
    angle = np.where(rng.random(n_kl) < 0.6, slope + rng.uniform(-0.05, 0.3, n_kl), np.arctan2(xy1[:, 1] - xy2[:, 1], xy1[:, 0] - xy2[:, 0]))
    kl = keylines(xy1, xy2, rng.integers(0, octaves, n_kl), angle.astype(F32))
    # the map lines' descriptors: noisy copies of a nearby keyline's (so windows hold true matches and competitors)
    mdesc = base.copy()
    kx = 0.5 * (xy1 + xy2)
    for i in range(m):
        q = _project(p, T, xyz[i]) if i < 4 * n_kl + 50 or i % 7 == 0 else None
        if few:
            k = int(rng.integers(0, min(few, n_kl))) if n_kl else -1
        elif q is not None and np.all(np.isfinite(q)) and n_kl:
            k = int(np.argmin(np.sum((kx - 0.5 * (q[:2] + q[2:])) ** 2, 1)))
        else:
            k = -1
        if k >= 0 and rng.random() < 0.9:
            mdesc[i] = desc_flip(rng, kdesc[k], int(rng.integers(0, 40)))
    u = rng.random(n_kl)
    cflags = np.where(u < preheld / 2, 3, np.where(u < preheld, 1, 0)).astype(np.uint8)
    cur = dict(kl=kl, desc=kdesc, flags=cflags)
    mflags = ((rng.random(m) < 0.9).astype(np.uint8)) | ((rng.random(m) < 0.7).astype(np.uint8) << 1)
    local = dict(xyz=xyz[:n_local], normal=normal[:n_local], dist=dd[:n_local], desc=mdesc[:n_local], flags=mflags[:n_local])
    return cur, local, T


def empty(d):
    return {k: v[:0] for k, v in d.items()}

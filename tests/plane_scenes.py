"""Synthetic plane-association and Manhattan-detection inputs (fixed seeds): a box room with three orthogonal wall families, map planes
with voxel-like clouds (0.2 m grid plus jitter), distractor planes, near-vertical and near-parallel planes, bad planes, empty and
NaN-holding clouds, frame planes that observe the walls from a camera pose, and Manhattan tables with full and partial entries whose
keyframes observe the walls (some keyframe indices -1).  Frames are manhattanslam_amd.plane dicts."""
import numpy as np

from tests import pose_scenes as ps

F32 = np.float32
PARAMS = dict(d_th=0.2, a_th=0.9, ver_th=0.08, par_th=0.9, mf_ver_th=0.1)


def params(**kw):
    p = dict(PARAMS)
    p.update(kw)
    return p


def _cloud(rng, n, d, center, n_pts, voxel=0.2, jitter=0.01):
    """n_pts points near the plane n.x + d = 0 around center, on a voxel-like grid."""
    u = np.cross(n, [1.0, 0, 0] if abs(n[0]) < 0.9 else [0, 1.0, 0]); u /= np.linalg.norm(u)
    v = np.cross(n, u)
    g = rng.integers(-8, 9, size=(n_pts, 2)) * voxel
    p = center + g[:, :1] * u + g[:, 1:] * v
    p = p - np.outer(p @ n + d, n) + rng.normal(size=(n_pts, 3)) * jitter
    return p.astype(F32)


def _plane(n, d):
    n = np.asarray(n, float)
    s = np.linalg.norm(n)
    return np.concatenate([n / s, [d / s]])


def room(seed, n_walls=6, n_distract=4, n_frame=None, pts=(20, 120), bad=0.1, empty=True, nan=True, n_kf=3, rot_deg=20.0,
         noise_deg=1.0, init_match=0.3, pose=None):
    """One frame.  Returns the frame dict and the true (R, t) of its mTcw.  pose: None, or a given true (R, t) of the camera (the room
    is then laid out around it)."""
    rng = np.random.default_rng(seed)
    Rw = ps.rot(rng.normal(size=3), rng.uniform(0, 90))                     # the room's Manhattan axes in the world
    if pose is not None:
        Rw = pose[0].T @ ps.rot(rng.normal(size=3), rng.uniform(0, rot_deg))
    walls = []
    for w in range(n_walls):
        ax = w % 3
        sgn = 1.0 if (w // 3) % 2 == 0 else -1.0
        walls.append(_plane(Rw[:, ax] * sgn, -rng.uniform(1.0, 3.0)))
    mp = list(walls)
    for _ in range(n_distract):
        kind = rng.integers(0, 3)
        if kind == 0:                                                       # random
            mp.append(_plane(rng.normal(size=3), rng.uniform(-3, 3)))
        elif kind == 1:                                                     # near-parallel to a wall, offset
            w = walls[rng.integers(len(walls))]
            n = ps.rot(rng.normal(size=3), rng.uniform(2, 15)) @ w[:3]
            mp.append(_plane(n, w[3] + rng.uniform(-1.5, 1.5)))
        else:                                                               # near-vertical to a wall
            w = walls[rng.integers(len(walls))]
            u = np.cross(w[:3], rng.normal(size=3))
            mp.append(_plane(ps.rot(rng.normal(size=3), rng.uniform(0, 4)) @ u, rng.uniform(-3, 3)))
    order = rng.permutation(len(mp))
    mp = [mp[o] for o in order]
    wall_idx = [int(np.flatnonzero(order == w)[0]) for w in range(n_walls)]
    M = len(mp)
    mp_w = np.array(mp, F32)
    flags = (rng.random(M) >= bad).astype(np.uint8)
    clouds = []
    for j in range(M):
        n, d = mp[j][:3].astype(float), float(mp[j][3])
        c = _cloud(rng, n, d, -d * n + rng.normal(size=3) * 0.5, int(rng.integers(pts[0], pts[1] + 1)))
        r = rng.random()
        if empty and r < 0.08:
            c = c[:0]
        elif nan and r < 0.2:
            c[rng.random(len(c)) < 0.3] = np.nan
        clouds.append(c)
    # the camera
    R = ps.rot(rng.normal(size=3), rng.uniform(0, rot_deg)) @ Rw.T
    t = rng.normal(size=3) * 0.3
    if pose is not None:
        R, t = np.asarray(pose[0], float), np.asarray(pose[1], float)
    Tcw = ps.tcw12(R, t)
    Twc = np.eye(4); Twc[:3, :3] = R.T; Twc[:3, 3] = -R.T @ t
    nf = n_frame if n_frame is not None else int(rng.integers(3, 10))
    seen = list(rng.permutation(M))[:nf]
    coef = []
    for j in seen:
        pc = Twc.T @ mp[j].astype(float)                                    # camera plane: Twc^T pi_w
        nn = ps.rot(rng.normal(size=3), rng.uniform(0, noise_deg)) @ pc[:3]
        coef.append(_plane(nn, pc[3] + rng.normal() * 0.02))
    for _ in range(int(rng.integers(0, 3))):                                # planes with no map counterpart
        coef.append(_plane(rng.normal(size=3), rng.uniform(-3, 3)))
    K = len(coef)
    coef = np.array(coef, F32).reshape(K, 4)
    pm = np.where(rng.random((K, 3)) < init_match, rng.integers(0, M, (K, 3)), -1).astype(np.int32)
    fr = dict(plane_coef=coef, Tcw=Tcw, plane_match=pm, plane_npts=rng.integers(10, 400, K).astype(np.int32), mp_w=mp_w, mp_flags=flags,
              mp_clouds=clouds)
    # keyframes observing every map plane at a permuted index (some not: -1), and the Manhattan tables over the walls
    kf_Rwc, kf_coef, kf_npts, kf_idx = [], [], [], []
    for _ in range(n_kf):
        Rk = ps.rot(rng.normal(size=3), rng.uniform(0, rot_deg)) @ Rw.T   # Rkw
        tk = rng.normal(size=3) * 0.3
        Tkw = np.eye(4); Tkw[:3, :3] = Rk; Tkw[:3, 3] = tk
        Twk = np.linalg.inv(Tkw)
        perm = rng.permutation(M)
        kc = np.zeros((M, 4), F32)
        for j in range(M):
            kc[perm[j]] = (Twk.T @ mp[j].astype(float)).astype(F32)
        kf_Rwc.append(Twk[:3, :3].astype(F32).reshape(9))
        kf_coef.append(kc)
        kf_npts.append(rng.integers(10, 400, M).astype(np.int32))
        kf_idx.append(np.where(rng.random(M) < 0.1, -1, perm))
    full, part, used_f, used_p = [], [], set(), set()
    fam = {w: w % 3 for w in range(n_walls)}
    for _ in range(int(rng.integers(2, 8))):
        a, b, c = (int(rng.integers(0, n_walls)) for _ in range(3))
        if len({fam[a], fam[b], fam[c]}) < 3:
            continue
        key = tuple(sorted((wall_idx[a], wall_idx[b], wall_idx[c])))
        if key in used_f:
            continue
        used_f.add(key)
        kf = int(rng.integers(0, n_kf))
        ms = [wall_idx[a], wall_idx[b], wall_idx[c]]
        full.append(ms + [kf] + [int(kf_idx[kf][m]) for m in ms])
    for _ in range(int(rng.integers(2, 10))):
        a, b = int(rng.integers(0, n_walls)), int(rng.integers(0, n_walls))
        if fam[a] == fam[b]:
            continue
        key = tuple(sorted((wall_idx[a], wall_idx[b])))
        if key in used_p:
            continue
        used_p.add(key)
        kf = int(rng.integers(0, n_kf))
        ms = [wall_idx[a], wall_idx[b]]
        part.append(ms + [kf] + [int(kf_idx[kf][m]) for m in ms])
    fr.update(full=np.array(full, np.int32).reshape(-1, 7), part=np.array(part, np.int32).reshape(-1, 5), kf_Rwc=np.array(kf_Rwc, F32),
              kf_coef=kf_coef, kf_npts=kf_npts)
    return fr, R, t

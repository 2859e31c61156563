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


# ---- hand-built frames: the reference's quirks, and the scenes of tests/test_plane_limits_gpu.py ------------------------------------------
IDENT = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
INT_MAX = 2 ** 31 - 1


def frame(coef, mp_w, clouds, flags=None, match=None, Tcw=None):
    coef = np.asarray(coef, F32).reshape(-1, 4)
    return dict(plane_coef=coef, Tcw=np.asarray(Tcw if Tcw is not None else IDENT, F32),
                plane_match=np.full((len(coef), 3), -1, np.int32) if match is None else np.asarray(match, np.int32),
                mp_w=np.asarray(mp_w, F32).reshape(-1, 4), mp_flags=np.ones(len(mp_w), np.uint8) if flags is None else np.asarray(flags, np.uint8),
                mp_clouds=[np.asarray(c, F32).reshape(-1, 3) for c in clouds], plane_npts=np.full(len(coef), 100, np.int32))


def mf_frame(coef, npts, full=(), part=(), kf_npts=None):
    """Frame planes i held by map plane i, one keyframe observing map plane q at index q with the same coefficients."""
    coef = np.asarray(coef, F32).reshape(-1, 4)
    K = len(coef)
    fr = frame(coef, coef, [[]] * K, match=[[i, -1, -1] for i in range(K)])
    fr.update(plane_npts=np.asarray(npts, np.int32), full=np.asarray(full, np.int32).reshape(-1, 7),
              part=np.asarray(part, np.int32).reshape(-1, 5), kf_Rwc=np.eye(3, dtype=F32).reshape(1, 9), kf_coef=[coef],
              kf_npts=[np.asarray(kf_npts if kf_npts is not None else [10] * K, np.int32)])
    return fr


AXES = [[1, 0, 0, -1], [0, 1, 0, -1], [0, 0, 1, -1], [0, 0, 1, -2]]
UP = [0, 0, 1, -1]                                                          # the frame plane z = 1 of most association frames


def association_quirks():
    """The hand-built association frames of tests/test_plane_model.py: [(name, frame, plane_match after the call, nmatches)] under PARAMS."""
    return [
        ("kept_vertical_only", frame([UP], [[1, 0, 0, 0]], [[[0, 0, 0]]], match=[[5, 7, 9]]), [[5, 7, 0]], 0),
        ("kept_everything", frame([UP], [[0.5, 0.5, 0.7071, 0]], [[[0, 0, 0]]], match=[[5, 7, 9]]), [[5, 7, 9]], 0),
        ("distance_fail_is_parallel", frame([UP], [[0, 0, 1, -3]], [[[0, 0, 3]]]), [[-1, 0, -1]], 0),
        ("bad_skipped", frame([UP], [[0, 0, 1, -1], [0, 0, 1, -1]], [[[0, 0, 1]], [[0, 0, 1.05]]], flags=[0, 1]), [[1, -1, -1]], 1),
        ("empty_cloud", frame([UP], [UP], [[]]), [[-1, 0, -1]], 0),
        ("first_wins", frame([UP], [UP] * 3 + [[1, 0, 0, 0]] * 2, [[[0, 0, 1.1]]] * 3 + [[[0, 0, 0]]] * 2), [[0, 1, 3]], 1),
    ]


def threshold_frames():
    """Frames that sit exactly on a threshold, from exactly representable floats: every comparison of the walk is strict, so none of them
    matches; one float further does.  [(name, frame, plane_match, nmatches)] under PARAMS with d_th = 0.25."""
    a, v = F32(PARAMS["a_th"]), F32(PARAMS["ver_th"])                       # a_th == par_th
    up = lambda x: float(np.nextafter(F32(x), F32(2)))
    near = [[0, 0, 1.0625]]                                                 # distance 0.0625 from z = 1
    return [
        ("angle_eq_a_th", frame([UP], [[0, 0, float(a), 0]], [near]), [[-1, -1, -1]], 0),   # not > a_th, not > par_th
        ("angle_above_a_th", frame([UP], [[0, 0, up(a), 0]], [near]), [[0, -1, -1]], 1),
        ("angle_eq_minus_par_th", frame([UP], [[0, 0, -float(a), 0]], [near]), [[-1, -1, -1]], 0),
        ("angle_below_minus_par_th", frame([UP], [[0, 0, -up(a), 0]], [near]), [[-1, 0, -1]], 0),
        ("angle_eq_ver_th", frame([UP], [[0, 0, float(v), 0], [0, 0, -float(v), 0]], [near] * 2), [[-1, -1, -1]], 0),
        ("angle_inside_ver_th", frame([UP], [[0, 0, float(np.nextafter(v, F32(0))), 0]], [near]), [[-1, -1, 0]], 0),
        ("distance_eq_d_th", frame([UP], [UP], [[[0, 0, 1.25]]]), [[-1, 0, -1]], 0),            # |1.25 - 1| == 0.25: falls through
        ("distance_below_d_th", frame([UP], [UP], [[[0, 0, 1.25], [0, 0, 1.2499999]]]), [[0, -1, -1]], 1),
    ]


def group_frames(counts=(1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64), n_map=12, seed=7000):
    """One frame per count of frame planes around the 16-plane groups of k_plane_dis: 12 good map planes seen from a camera pose; frame
    plane k observes map plane k % 12 (and matches it), except every fifth plane of the frames that are not the first or the last, which
    is a random plane.  So the last frame's planes all match and the first frame's single plane does."""
    rng = np.random.default_rng(seed)
    mp = [_plane(rng.normal(size=3), rng.uniform(-3, 3)) for _ in range(n_map)]
    clouds = [_cloud(rng, p[:3], p[3], -p[3] * p[:3], 5 + 3 * j) for j, p in enumerate(mp)]
    frames = []
    for c, K in enumerate(counts):
        R, t = ps.rot(rng.normal(size=3), rng.uniform(0, 40)), rng.normal(size=3) * 0.3
        Twc = np.eye(4); Twc[:3, :3] = R.T; Twc[:3, 3] = -R.T @ t
        coef = []
        for k in range(K):
            if k % 5 == 4 and 0 < c < len(counts) - 1:
                coef.append(_plane(rng.normal(size=3), rng.uniform(-3, 3)))
            else:
                coef.append(Twc.T @ mp[k % n_map])
        frames.append(frame(coef, mp, clouds, Tcw=ps.tcw12(R, t)))
    return frames


PROBE = dict(PARAMS, d_th=150.0)                                            # above 100: an empty cloud's distance is a match as well


def probe_map(specs, seed):
    """Map planes z = 1 + 0.01 j whose clouds are far (z in [10, 11), distance about 9) but for one point exactly on the plane.
    specs[j] = (points, position of that point or None, positions holding a NaN)."""
    rng = np.random.default_rng(seed)
    mp_w, clouds = [], []
    for j, (n, pos, nans) in enumerate(specs):
        z = F32(1 + 0.01 * j)
        c = np.concatenate([rng.uniform(-1, 1, (n, 2)), rng.uniform(10, 11, (n, 1))], 1).astype(F32)
        if pos is not None:
            c[pos, 2] = z
        for q in nans:
            c[q, (j + q) % 3] = np.nan
        mp_w.append([0, 0, 1, -float(z)])
        clouds.append(c)
    return mp_w, clouds


def probe_frame(pmap, targets):
    """Frame planes z = 1 + 0.01 t + 0.003, t in targets: the nearest cloud point of all is map plane t's one point (0.003 away, the
    neighbours' 0.007 and 0.013), and the distances shrink towards t, so slot 0 ends at t only if every minimum before it was right."""
    mp_w, clouds = pmap
    return frame([[0, 0, 1, -(float(F32(1 + 0.01 * t)) + 0.003)] for t in targets], mp_w, clouds)


def lane_frames(n=64, per_frame=17, seed=7100):
    """The wave minimum in every lane: n map planes whose clouds hold n points with the minimum of cloud L at point L (lane L of the
    first stride), probed by frames of per_frame planes (two groups) whose targets cover every L.  [(frame, targets)]."""
    pmap = probe_map([(n, L, ()) for L in range(n)], seed)
    order = np.random.default_rng(seed).permutation(n).tolist()
    order += order[:(-len(order)) % per_frame]
    return [(probe_frame(pmap, order[s:s + per_frame]), order[s:s + per_frame]) for s in range(0, len(order), per_frame)]


def stride_frame(sizes=(0, 1, 63, 65, 127, 128, 129, 1000), seed=7200):
    """Clouds of the given sizes with the minimum at the first point, at the last point and in the tail after the last full stride of 64;
    one frame plane per cloud that has one.  (frame, targets)."""
    specs = []
    for n in sizes:
        pos = {0, n - 1, 64 * ((n - 1) // 64) + ((n - 1) % 64) // 2} if n else {None}
        specs += [(n, p, ()) for p in sorted(pos, key=lambda x: -1 if x is None else x)]
    targets = [j for j, s in enumerate(specs) if s[1] is not None]
    return probe_frame(probe_map(specs, seed), targets), targets


def nan_lane_frames(n=64, per_frame=17, seed=7300):
    """Clouds of 2 n points with a NaN in every lane position: in the first half of the frames lane L reads its minimum first and a NaN
    after it, in the second half the NaN first.  [(frame, targets)]."""
    out = []
    for first in (True, False):
        pmap = probe_map([(2 * n, L if first else n + L, (n + L if first else L,)) for L in range(n)], seed + first)
        order = np.random.default_rng(seed).permutation(n).tolist()
        order += order[:(-len(order)) % per_frame]
        out += [(probe_frame(pmap, order[s:s + per_frame]), order[s:s + per_frame]) for s in range(0, len(order), per_frame)]
    return out


def nonfinite_frames():
    """[(name, frame, plane_match, nmatches)] under PROBE: an all-NaN cloud and an all-far cloud give 100 (a match below d_th = 150, no
    match at 100 < 100), +-Inf points give an Inf or NaN distance, a NaN coefficient or an Inf in Tcw makes every comparison false."""
    inf, nan = np.inf, np.nan
    mp_w = [UP, UP, UP, UP]
    clouds = [[[nan, 0, 1], [0, nan, 1], [0, 0, nan]], [[0, 0, 500], [0, 0, -400]], [[0, 0, inf], [0, 0, -inf], [inf, 0, 1]], [[0, 0, 1.05]]]
    return [
        ("clouds", frame([UP], mp_w, clouds), [[3, 1, -1]], 1),
        ("nan_coef", frame([UP, [nan, 0, 1, -1], [0, 0, 1, nan]], mp_w, clouds, match=[[-1, -1, -1], [1, 5, 0], [4, -1, 2]]),
         [[3, 1, -1], [1, 5, 0], [4, -1, 2]], 1),
        ("inf_tcw", frame([UP, [0, 1, 0, -1]], mp_w, clouds, match=[[2, 9, -1], [-1, 3, 3]], Tcw=[inf] + IDENT[1:]),
         [[2, 9, -1], [-1, 3, 3]], 0),
    ]


def csr_frame(seed=7400, n_map=9, n_pts=40):
    """A probe-style frame whose clouds are given by raw CSR offsets: (frame without clouds, points (n_pts, 3), offsets (n_map + 1,)) with
    negative offsets, offsets beyond the points, a decreasing pair and overlapping ranges.  The clouds follow from include/msl.h's rule."""
    rng = np.random.default_rng(seed)
    pts = np.concatenate([rng.uniform(-1, 1, (n_pts, 2)), rng.uniform(1, 3, (n_pts, 1))], 1).astype(F32)
    off = np.array([-5, 12, 4, 20, 31, n_pts + 100, n_pts + 200, 3, 9, 9 + 17], np.int32)[:n_map + 1]
    fr = frame([[0, 0, 1, -z] for z in np.linspace(1.1, 2.9, 17)], [UP] * n_map, [[]] * n_map)
    return fr, pts, off


def csr_clouds(pts, off, ptcap):
    """include/msl.h: b = clamp(off[j], 0, ptcap), e = clamp(off[j + 1], b, ptcap), cloud j = points [b, e)."""
    clouds = []
    for j in range(len(off) - 1):
        b = min(max(int(off[j]), 0), ptcap)
        e = min(max(int(off[j + 1]), b), ptcap)
        clouds.append(pts[b:e])
    return clouds


def cut(fr, K=None, M=None):
    """The frame with its first K frame planes and first M map planes only."""
    fr = dict(fr)
    if K is not None:
        for k in ("plane_coef", "plane_match", "plane_npts"):
            fr[k] = fr[k][:K]
    if M is not None:
        for k in ("mp_w", "mp_flags"):
            fr[k] = fr[k][:M]
        fr["mp_clouds"] = fr["mp_clouds"][:M]
    return fr


def big_map_frame(M=4096, K=64, seed=7500):
    """M map planes (one in ten bad, clouds of 1..8 points up to 0.3 off their plane) seen from a camera pose by K frame planes: plane 0
    observes map plane M - 1, plane 1 map plane 0, plane 2 map plane M - 2 (good planes with a point exactly on them: they win slot 0),
    every other even plane a random map plane, every odd one a random plane."""
    rng = np.random.default_rng(seed)
    n = rng.normal(size=(M, 3)); n /= np.linalg.norm(n, axis=1, keepdims=True)
    d = rng.uniform(-3, 3, M)
    flags = (rng.random(M) >= 0.1).astype(np.uint8)
    clouds = []
    for j in range(M):
        c = 1 + (j * 5) % 8
        p = rng.normal(size=(c, 3))
        p += np.outer(rng.uniform(-0.3, 0.3, c) - (p @ n[j] + d[j]), n[j])
        clouds.append(p.astype(F32))
    wins = [M - 1, 0, M - 2]
    for j in wins:
        flags[j] = 1
        clouds[j][-1] = (clouds[j][-1].astype(float) - (clouds[j][-1].astype(float) @ n[j] + d[j]) * n[j]).astype(F32)
    mp = np.concatenate([n, d[:, None]], 1)
    R, t = ps.rot(rng.normal(size=3), 25.0), rng.normal(size=3) * 0.3
    Twc = np.eye(4); Twc[:3, :3] = R.T; Twc[:3, 3] = -R.T @ t
    coef = []
    for k in range(K):
        if k < 3:
            coef.append(Twc.T @ mp[wins[k]])
        elif k % 2 == 0:
            coef.append(Twc.T @ mp[rng.integers(M)])
        else:
            coef.append(_plane(rng.normal(size=3), rng.uniform(-3, 3)))
    pm = np.where(rng.random((K, 3)) < 0.3, rng.integers(0, M, (K, 3)), -1).astype(np.int32)
    return frame(coef, mp, clouds, flags=flags, match=pm, Tcw=ps.tcw12(R, t)), wins


def huge_cloud_frame(P=1 << 22, K=17, seed=7600):
    """Two map planes: plane 0 with an empty cloud, plane 1 with P points about 9 away whose very last point lies at z = 1.5.  Frame
    planes z = 1 + 0.06 k: under d_th = 0.5 plane k matches map plane 1 exactly when |0.5 - 0.06 k| < 0.5, that is for 0 < k <= 16."""
    rng = np.random.default_rng(seed)
    c = np.empty((P, 3), F32)
    c[:, :2] = rng.random((P, 2), F32)
    c[:, 2] = 10 + rng.random(P, F32)
    c[-1, 2] = 1.5
    return frame([[0, 0, 1, -(1 + 0.06 * k)] for k in range(K)], [UP, UP], [np.zeros((0, 3), F32), c])


def wide_association_batch(n=300, seed=7700):
    """n small room() frames, more than the device has compute units, with hand-built frames of known answers at 0, 255, 256 and n - 1.
    (frames, {index: (plane_match, nmatches)})."""
    frames = [room(seed + f, pts=(0, 12))[0] for f in range(n)]
    q = {x[0]: x for x in association_quirks()}
    known = {}
    for f, name in ((0, "kept_vertical_only"), (255, "first_wins"), (256, "distance_fail_is_parallel"), (n - 1, "bad_skipped")):
        frames[f] = q[name][1]
        known[f] = q[name][2:]
    return frames, known


# ---- Manhattan detection ---------------------------------------------------------------------------------------------------------------
def manhattan_quirks():
    """The hand-built detection frames of tests/test_plane_model.py: [(name, frame, found, full, choice[:3] or None)]."""
    pair3 = [[0, 1, 0, 0, 1], [0, 2, 0, 0, 2], [1, 2, 0, 1, 2]]
    return [
        ("pair_replaces_triple", mf_frame(AXES, [10, 10, 10, 500], full=[[0, 1, 2, 0, 0, 1, 2]], part=[[1, 3, 0, 1, 3]]), 1, 0, [1, 3, -1]),
        ("triple_stays", mf_frame(AXES, [10, 10, 10, 5], full=[[0, 1, 2, 0, 0, 1, 2]], part=[[1, 3, 0, 1, 3]]), 1, 1, [0, 1, 2]),
        ("first_maximum", mf_frame(AXES, [10, 10, 10, 10], part=pair3), 1, 0, [0, 1, -1]),
        ("minus_one_skips", mf_frame(AXES, [10, 10, 10, 10], part=[[0, 1, 0, -1, 1], [0, 2, 0, 0, 2]]), 1, 0, [0, 2, -1]),
        ("partial_flip", mf_frame([[0, 1, 0, -1], [1, 0, 0, -1]], [10, 10], part=[[0, 1, 0, 0, 1]]), 1, 0, [0, 1, -1]),
        ("full_left_handed", mf_frame([[0, 1, 0, -1], [1, 0, 0, -1], [0, 0, 1, -1]], [10, 10, 10], full=[[0, 1, 2, 0, 0, 1, 2]]), 1, 1,
         [0, 1, 2]),
        ("nothing", mf_frame(AXES, [10, 10, 10, 10]), 0, 0, None),
    ]


def _add_keyframes(fr, counts):
    """Further keyframe slots observing the same planes, slot 1 + q with counts[q] points on every plane."""
    K = len(fr["plane_coef"])
    fr["kf_Rwc"] = np.tile(fr["kf_Rwc"][:1], (1 + len(counts), 1))
    fr["kf_coef"] = [fr["kf_coef"][0]] * (1 + len(counts))
    fr["kf_npts"] = [fr["kf_npts"][0]] + [np.full(K, c, np.int32) for c in counts]
    return fr


def tie_frame(n=64, variant=None):
    """n frame planes of three axis families (plane k: family k % 3, sign alternating, its own offset), each held by its own map plane;
    every count is 10 and the tables hold every cross-family triple and pair, so every triple scores 60 and every pair 40: the first
    triple (0, 1, 2) wins by order alone.  Variants move table rows to keyframe slots with other counts (slot 1: 11, 2: 21, 3: 26,
    4: 14 points per plane):
      a  the last triple in loop order -> slot 1: 63, the unique maximum
      b  the pair (n - 2, n - 1) -> slot 2: 62, the unique maximum and the largest order value
      c  the pair (3, 4) -> slot 3 and the later triple (3, 5, 7) -> slot 4: both 72, the pair is first
      d  the triple (3, 4, 5) -> slot 4 and its own pair (3, 4) -> slot 3: both 72, the triple is first
    Returns (frame, expected choice[:3])."""
    fam = [k % 3 for k in range(n)]
    coef = np.zeros((n, 4), F32)
    for k in range(n):
        coef[k, fam[k]] = 1 if (k // 3) % 2 == 0 else -1
        coef[k, 3] = -(1 + 0.1 * k)
    triples = [(a, b, c) for a in range(n) for b in range(a + 1, n) for c in range(b + 1, n) if len({fam[a], fam[b], fam[c]}) == 3]
    pairs = [(a, b) for a in range(n) for b in range(a + 1, n) if fam[a] != fam[b]]
    slot_f, slot_p, want = {}, {}, [0, 1, 2]
    if variant == "a":
        slot_f[triples[-1]] = 1; want = list(triples[-1])
    elif variant == "b":
        slot_p[(n - 2, n - 1)] = 2; want = [n - 2, n - 1, -1]
    elif variant == "c":
        slot_p[(3, 4)] = 3; slot_f[(3, 5, 7)] = 4; want = [3, 4, -1]
    elif variant == "d":
        slot_f[(3, 4, 5)] = 4; slot_p[(3, 4)] = 3; want = [3, 4, 5]
    full = [[a, b, c, slot_f.get((a, b, c), 0), a, b, c] for a, b, c in triples]
    part = [[a, b, slot_p.get((a, b), 0), a, b] for a, b in pairs]
    return _add_keyframes(mf_frame(coef, [10] * n, full=full, part=part), [11, 21, 26, 14]), want


def score_frames():
    """[(name, frame, found, choice[:3] or None, score)]: a score of exactly 2^31 - 1 (no partial sum of the kernel's left-to-right int
    additions overflows) against one of 2^31 - 2, in both loop orders; candidates scoring exactly 0 and below 0 are no candidates."""
    third = 715827882                                                       # 3 * third = 2^31 - 2
    half = 1073741822                                                       # 2 * half = 2^31 - 4
    out = []
    for name, npts, want, score in (("max_first", [1, 0, 0, 2], [0, 1, 2], INT_MAX), ("max_later", [0, 0, 0, 3], [1, 3, -1], INT_MAX)):
        fr = mf_frame(AXES, npts, full=[[0, 1, 2, 0, 0, 1, 2]], part=[[1, 3, 1, 1, 3]], kf_npts=[third] * 3 + [0])
        _add_keyframes(fr, [half])
        out.append((name, fr, 1, want, score))
    rows = [[0, 1, 0, 0, 1], [0, 2, 1, 0, 2], [1, 2, 2, 1, 2]]               # scores 0, -10 and 6
    for name, part, found, want, score in (("zero_and_negative_lose", rows, 1, [1, 2, -1], 6), ("only_zero_and_negative", rows[:2], 0, None, 0)):
        fr = mf_frame(AXES, [0, 0, 0, 0], part=part, kf_npts=[0] * 4)
        _add_keyframes(fr, [-5, 3])
        out.append((name, fr, found, want, score))
    return out


def big_table_frame(fcap=65536, qcap=65536, mcap=4096, kcap=4096, pcap=64, seed=7800):
    """12 frame planes (family k % 3) holding map planes 0, 1, 2, three around mcap / 2, three around mcap / 4 and mcap - 3 .. mcap - 1,
    with both tables full: fcap / qcap strictly ascending keys over [0, mcap).  The frame's own keys sit at row 0 ((0, 1, 2) and (0, 1)),
    at the last row ((mcap - 3, mcap - 2, mcap - 1) and (mcap - 2, mcap - 1)) and mid-table, beside keys that differ from them in the
    last component only.  The last full row names keyframe slot kcap - 1 and that keyframe's planes 0, pcap - 1 and 5 with 1000 points
    each: it wins; the last partial row (slot kcap - 2, 900 points) is the best pair.  Returns (frame, row indices of the own keys
    {"full": [...], "part": [...]})."""
    rng = np.random.default_rng(seed)
    h, q = mcap // 2, mcap // 4
    held = [0, 1, 2, h - 1, h, h + 1, q - 1, q, q + 1, mcap - 3, mcap - 2, mcap - 1]
    K = len(held)
    coef = np.zeros((K, 4), F32)
    for k in range(K):
        coef[k, k % 3] = 1
        coef[k, 3] = -(1 + 0.1 * k)
    own_f = [(0, 1, 2), (q - 1, q, q + 1), (mcap - 3, mcap - 2, mcap - 1)]    # sorted random triples put a first component mcap / 4 mid-table
    own_p = [(0, 1), (q - 1, q), (mcap - 2, mcap - 1)]
    miss_f = [(0, 1, 3), (q - 1, q, q + 2), (q - 1, q, q), (mcap - 3, mcap - 2, mcap - 2), (mcap - 4, mcap - 2, mcap - 1)]
    miss_p = [(0, 3), (q - 1, q + 2), (q - 1, q - 1), (mcap - 2, mcap - 2), (mcap - 3, mcap - 1)]

    def table(w, cap, own, miss):
        keys = set(own) | set(miss)
        while len(keys) < cap:
            draw = np.sort(rng.integers(0, mcap, (2 * cap, w)), axis=1)
            draw = draw[(np.diff(draw, axis=1) > 0).all(1)]
            for row in draw.tolist():
                keys.add(tuple(row))
                if len(keys) == cap:
                    break
        keys = sorted(keys)
        tab = np.zeros((cap, 2 * w + 1), np.int32)
        tab[:, :w] = keys
        tab[:, w] = rng.integers(0, max(kcap - 2, 1), cap)
        tab[:, w + 1:] = rng.integers(0, pcap, (cap, w))
        return tab, [keys.index(k) for k in own]
    full, rows_f = table(3, fcap, own_f, miss_f)
    part, rows_p = table(2, qcap, own_p, miss_p)
    full[rows_f[-1], 3:] = [kcap - 1, 0, pcap - 1, 5]
    part[rows_p[-1], 2:] = [kcap - 2, 7, 3]
    kn = rng.integers(1, 50, (kcap, pcap)).astype(np.int32)
    kn[kcap - 1], kn[kcap - 2] = 1000, 900
    kc = np.zeros((kcap, pcap, 4), F32)
    for slot, idx, planes in ((kcap - 1, (0, pcap - 1, 5), (9, 10, 11)), (kcap - 2, (7, 3), (10, 11))):
        for i, p in zip(idx, planes):
            kc[slot, i] = coef[p]
    flags = np.ones(mcap, np.uint8)
    fr = dict(plane_coef=coef, Tcw=np.asarray(IDENT, F32), plane_match=np.array([[m, -1, -1] for m in held], np.int32),
              plane_npts=rng.integers(10, 400, K).astype(np.int32), mp_w=np.zeros((mcap, 4), F32), mp_flags=flags,
              mp_clouds=[np.zeros((0, 3), F32)] * mcap, full=full, part=part,
              kf_Rwc=np.tile(ps.rot([1.0, 2.0, 3.0], 30.0).astype(F32).reshape(1, 9), (kcap, 1)), kf_coef=list(kc), kf_npts=list(kn))
    return fr, dict(full=rows_f, part=rows_p)


GATES = ("index_minus_one", "index_pcap", "slot_minus_one", "slot_kcap", "match_minus_one", "match_n_map", "match_int_max", "bad_plane",
         "full_index_beyond_pcap")


def gate_frame(repair=None):
    """20 frame planes (family k % 3), 40 map planes, 3 keyframe slots (slot 1 with 500000 points per plane).  Planes 2 and 3 both hold
    map plane 5 and the partial table has the row (5, 5): it is the winner (score 620) ahead of the plain pair (0, 1) (220).  Every other
    entry names slot 1 and so would score a million, but is no candidate -- one reason each, in GATES order: the pairs (4, 5), (6, 7),
    (8, 9), (10, 11) by their entries (a keyframe plane index -1 or pcap, a slot -1 or kcap), the pairs (12, 13), (14, 15), (16, 17) by
    plane 12 / 14 / 16's slot-0 plane_match (-1, n_map, 2^31 - 1: their rows are keyed by exactly those values), (18, 19) by plane 18's
    map plane being bad, and the triple (4, 5, 6) by a keyframe plane index beyond pcap.  repair: one GATES name whose reason is taken
    away; that candidate then wins.  Returns (frame, expected choice[:3])."""
    K, M = 20, 40
    coef = np.zeros((K, 4), F32)
    for k in range(K):
        coef[k, k % 3] = 1
        coef[k, 3] = -(1 + 0.1 * k)
    held = [0, 1, 5, 5] + [10 + p for p in range(4, K)]
    bad = {"index_minus_one": (4, [14, 15, 1, -1, 3]), "index_pcap": (6, [16, 17, 1, 2, K]), "slot_minus_one": (8, [18, 19, -1, 1, 2]),
           "slot_kcap": (10, [20, 21, 3, 1, 2])}
    part = [[0, 1, 0, 0, 1], [5, 5, 0, 2, 3]]
    for name, (p, row) in bad.items():
        part.append([10 + p, 11 + p, 1, 1, 2] if name == repair else row)
    flags = np.ones(M, np.uint8)
    for name, p, value in (("match_minus_one", 12, -1), ("match_n_map", 14, M), ("match_int_max", 16, INT_MAX), ("bad_plane", 18, 28)):
        if name != repair:
            held[p] = value
            flags[28] = 0 if name == "bad_plane" else flags[28]
        part.append([held[p], held[p + 1], 1, 1, 2])
    full = [[14, 15, 16, 1, 0, 1, 2 if repair == "full_index_beyond_pcap" else K + 3]]
    fr = mf_frame(coef, [10] * K, full=full, part=part, kf_npts=[100, 100, 300] + [100] * (K - 3))
    _add_keyframes(fr, [500000, 7])
    fr.update(plane_match=np.array([[m, -1, -1] for m in held], np.int32), mp_w=np.zeros((M, 4), F32), mp_flags=flags,
              mp_clouds=[np.zeros((0, 3), F32)] * M)
    if repair is None:
        want = [2, 3, -1]
    elif repair == "full_index_beyond_pcap":
        want = [4, 5, 6]
    else:
        want = [4 + 2 * GATES.index(repair), 5 + 2 * GATES.index(repair), -1]
    return fr, want


def polar_frames(n=24, seed=7900):
    """Frames whose keyframe normals are neither orthogonal nor unit length (pairwise angles 60..120 degrees, lengths 0.25..4) while the
    frame's own planes are a slightly perturbed orthonormal triple: full triples of either handedness on the keyframe side (even frames
    right-handed, frames 1 mod 4 left-handed) and partial pairs (frames 3 mod 4) in either order.  Returns [(frame, kind)]."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        f = len(out)
        Rc = ps.rot(rng.normal(size=3), rng.uniform(0, 180)) @ ps.rot(rng.normal(size=3), 1.0)
        c = np.array([ps.rot(rng.normal(size=3), rng.uniform(0, 1.5)) @ Rc[:, q] for q in range(3)])
        Q = ps.rot(rng.normal(size=3), rng.uniform(0, 180))
        m = np.array([ps.rot(rng.normal(size=3), rng.uniform(0, 17)) @ Q[:, q] for q in range(3)])
        cs = [m[a] @ m[b] for a, b in ((0, 1), (0, 2), (1, 2))]
        if max(abs(x) for x in cs) > 0.5:                                   # 60 .. 120 degrees
            continue
        m *= rng.uniform(0.25, 4.0, (3, 1))
        kind = "partial" if f % 4 == 3 else ("left" if f % 4 == 1 else "right")
        if kind == "left":
            m[2] = -m[2]
        if kind == "partial" and f % 8 == 7:
            m[[0, 1]] = m[[1, 0]]
        coef = np.concatenate([c, -rng.uniform(1, 3, (3, 1))], 1)
        kc = np.concatenate([m, -rng.uniform(1, 3, (3, 1))], 1).astype(F32)
        if kind == "partial":
            fr = mf_frame(coef[:2], [10, 10], part=[[0, 1, 0, 0, 1]])
            kc = kc[:2]
        else:
            fr = mf_frame(coef, [10, 10, 10], full=[[0, 1, 2, 0, 0, 1, 2]])
        fr.update(kf_coef=[kc], kf_Rwc=ps.rot(rng.normal(size=3), rng.uniform(0, 180)).astype(F32).reshape(1, 9))
        out.append((fr, kind))
    return out


def wide_manhattan_batch(n=300, seed=8000):
    """n small associated room() frames with hand-built frames of known answers at 0, 255, 256 and n - 1.
    (frames, {index: (found, full, choice[:3] or None)})."""
    from tests import plane_match_model as pmm
    frames = []
    for f in range(n):
        fr = room(seed + f, pts=(0, 6), n_frame=int(6 + f % 5))[0]
        frames.append(dict(fr, plane_match=pmm.search_fast(fr, PARAMS)[1]))
    q = {x[0]: x for x in manhattan_quirks()}
    known = {}
    for f, name in ((0, "pair_replaces_triple"), (255, "minus_one_skips"), (256, "nothing"), (n - 1, "full_left_handed")):
        frames[f] = q[name][1]
        known[f] = q[name][2:]
    return frames, known

"""Inputs for the relocalisation tests (the keyframe search): hand-made pairs for the model's first-principles tests and seeded random
pairs for the GPU parity tests.  Per-pair dicts as manhattanslam_amd.reloc.pack_keyframe_points takes them; cameras and grids are those
of tests/match_scenes.py and tests/local_match_scenes.py."""
import math

import numpy as np

from tests import local_match_scenes as ls
from tests import match_scenes as ms

KEYPOINT_DTYPE = ms.KEYPOINT_DTYPE


def params(th=10.0, orb_dist=100, check_orientation=True, nlevels=8, scale=1.2, **kw):
    from manhattanslam_amd import KEYFRAME_MATCH_PARAMS_DTYPE
    p = ms.params(None, th, check_orientation, dtype=KEYFRAME_MATCH_PARAMS_DTYPE, nlevels=nlevels, scale=scale, **kw)
    p["log_scale_factor"], p["orb_dist"] = np.float32(math.log(scale)), orb_dist
    return p


def frame(p, kps):
    """kps: list of (x, y, octave, hamming distance to the zero descriptor, angle, held)."""
    n = len(kps)
    k = np.zeros(n, KEYPOINT_DTYPE)
    xy = np.array([[a[0], a[1]] for a in kps], np.float32).reshape(n, 2)
    k["x"], k["y"] = xy[:, 0], xy[:, 1]
    k["octave"] = [a[2] for a in kps]
    k["angle"] = [a[4] for a in kps]
    k["class_id"] = -1
    return dict(kps=k, un_xy=xy, grid_cell=ms.grid_cells(xy, p), desc=np.stack([ls.desc_at(a[3]) for a in kps]) if n else np.zeros((0, 32), np.uint8),
                held=np.array([a[5] for a in kps], np.uint8))


def keyframe(pts):
    """pts: list of (xyz, (mfMinDistance, mfMaxDistance), angle, flags); every point has the all-zero descriptor."""
    m = len(pts)
    return dict(xyz=np.array([a[0] for a in pts], np.float32).reshape(m, 3), dist=np.array([a[1] for a in pts], np.float32).reshape(m, 2),
                desc=np.zeros((m, 32), np.uint8), angle=np.array([a[2] for a in pts], np.float32), flags=np.array([a[3] for a in pts], np.uint8))


def pixel_point(p, u, v, z):
    """The camera-frame point (identity pose: also the world point) that projects to (u, v) at depth z (z < 0: behind the camera)."""
    fx, fy, cx, cy = (float(p[k][0]) for k in ("fx", "fy", "cx", "cy"))
    return ((u - cx) * z / fx, (v - cy) * z / fy, z)


def random_pair(seed, p, n_cur=700, n_kf=650, held=0.2, cluster=False, conflict=False, identity=False, desc_noise=10):
    """A current frame of n_cur keypoints and a keyframe of n_kf map points under a random pose.  Most keyframe points project next to a
    keypoint whose octave is near the point's predicted level, with a noisy copy of its descriptor and an angle a few degrees off (one in
    seven: any angle, for the rotation check); 3 % lie behind the camera on the same ray (same projection, no depth test in this search),
    2 % outside the image, 2 % outside their distance range, 10 % are not candidates (kf_flags 0).  cluster: everything in a small region
    (windows beyond the 32 stored candidates); conflict: many points share a few keypoints and descriptors (earlier queries take later
    queries' best: many fixpoint rounds); identity: the identity pose, with a few points at depth exactly 0 (NaN / infinite projection)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    fx, fy, cx, cy = (float(p[k][0]) for k in ("fx", "fy", "cx", "cy"))
    W, H = float(p["maxX"][0]), float(p["maxY"][0])
    nlevels, scale = int(p["nlevels"][0]), ms.level_scale(p)
    T = np.eye(4, dtype=np.float32)
    if not identity:
        T[:3, :3], T[:3, 3] = ls.rotation(rng, 8.0), rng.normal(0, 0.3, 3)
    T64 = T.astype(np.float64)
    Rwc, Ow = T64[:3, :3].T, -T64[:3, :3].T @ T64[:3, 3]
    if cluster:
        xy = np.stack([rng.uniform(120, 520, n_cur), rng.uniform(90, 390, n_cur)], 1)
    else:
        xy = np.stack([rng.uniform(2, W - 2, n_cur), rng.uniform(2, H - 2, n_cur)], 1)
    xy = np.round(xy * 4).astype(np.float32) / 4
    depth = rng.uniform(0.8, 6.0, n_cur)
    kps = np.zeros(n_cur, KEYPOINT_DTYPE)
    kps["x"], kps["y"] = xy[:, 0], xy[:, 1]
    kps["octave"] = rng.integers(0, nlevels, n_cur)
    kps["angle"] = rng.uniform(0, 360, n_cur).astype(np.float32)
    kps["class_id"] = -1
    desc = rng.integers(0, 256, (n_cur, 32), dtype=np.uint8)
    if conflict and n_cur:
        desc = desc[rng.integers(0, 6, n_cur)]
    nt = n_cur // 6                                                      # twins: the last sixth sits next to an earlier keypoint, same octave, near-equal
    if nt:                                                               # descriptor -- the fall-back of a query whose best is held or already taken
        tw = rng.integers(0, n_cur - nt, nt)
        xy[n_cur - nt:] = xy[tw] + np.round(rng.uniform(-1.5, 1.5, (nt, 2)) * 4).astype(np.float32) / 4
        kps["x"], kps["y"] = xy[:, 0], xy[:, 1]
        kps["octave"][n_cur - nt:] = kps["octave"][tw]
        desc[n_cur - nt:] = desc[tw]
        bit = rng.integers(0, 256, (nt, 4))
        for k in range(4):
            desc[n_cur - nt + np.arange(nt), bit[:, k] // 8] ^= (1 << (bit[:, k] % 8)).astype(np.uint8)
    cur = dict(kps=kps, un_xy=xy, grid_cell=ms.grid_cells(xy, p), desc=desc, held=(rng.random(n_cur) < held).astype(np.uint8))
    m = max(n_kf, 1)
    if n_cur:
        src = rng.integers(0, min(n_cur, 150) if conflict else n_cur, m)
        uu = xy[src, 0] + rng.normal(0, 1.0, m); vv = xy[src, 1] + rng.normal(0, 1.0, m); zz = depth[src] * rng.uniform(0.97, 1.03, m)
        lvl = np.clip(kps["octave"][src] + rng.integers(-1, 2, m), 0, nlevels - 1)
        kdesc = desc[src].copy()
        off = np.where(rng.random(m) < 6 / 7, rng.normal(3.0, 2.0, m), rng.uniform(0, 360, m))
        angle = (kps["angle"][src] + off) % 360
    else:
        uu = rng.uniform(0, W, m); vv = rng.uniform(0, H, m); zz = rng.uniform(1, 5, m)
        lvl = rng.integers(0, nlevels, m)
        kdesc = rng.integers(0, 256, (m, 32), dtype=np.uint8)
        angle = rng.uniform(0, 360, m)
    Pc = np.stack([(uu - cx) * zz / fx, (vv - cy) * zz / fy, zz], 1)
    kind = rng.random(m)
    Pc[kind < 0.03] *= -1                                                # behind the camera, same projection
    out = (kind >= 0.03) & (kind < 0.05)
    Pc[out, 0] += zz[out] * 2.0                                          # out of the image
    if identity:
        zero = (kind >= 0.05) & (kind < 0.08)
        Pc[zero, 2] = 0.0                                                # zc == 0: infinite u / v ...
        Pc[zero & (rng.random(m) < 0.5), 0] = 0.0                        # ... or 0 * inf = NaN
    Pw = (Rwc @ Pc.T).T + Ow
    dist = np.linalg.norm(Pw - Ow, axis=1)
    # a distance range that predicts about level lvl: mfMaxDistance = dist * scale^(lvl - frac); 5 % predict a level beyond the top of the pyramid (clamped)
    far = rng.random(m)
    lv = np.where(far < 0.05, nlevels + 2.0, lvl.astype(np.float64))
    dmax = dist * scale ** (lv - rng.uniform(0.05, 0.95, m))
    dmin = np.where(far < 0.05, 0.0, dmax / scale ** (nlevels - 1))
    rng_out = (kind >= 0.08) & (kind < 0.10)
    dmax[rng_out] = dist[rng_out] / 1.3                                   # beyond 1.2 * mfMaxDistance
    flip = rng.integers(0, 256, (m, desc_noise))
    for k in range(desc_noise):
        kdesc[np.arange(m), flip[:, k] // 8] ^= (1 << (flip[:, k] % 8)).astype(np.uint8)
    unrelated = rng.random(m) < 0.1
    kdesc[unrelated] = rng.integers(0, 256, (int(unrelated.sum()), 32), dtype=np.uint8)
    kf = dict(xyz=Pw.astype(np.float32), dist=np.stack([dmin, dmax], 1).astype(np.float32), desc=kdesc, angle=angle.astype(np.float32),
              flags=(rng.random(m) < 0.9).astype(np.uint8))
    if n_kf == 0:
        kf = {k: v[:0] for k, v in kf.items()}
    return cur, kf, T


N_CUR = [0, 1, 300, 97, 640, 5, 700, 64]
N_KF = [200, 300, 0, 130, 600, 7, 650, 1]


def ragged_batch(p):
    """The main GPU scene: 8 ragged pairs, among them an empty frame, an empty keyframe, a clustered, a conflict-heavy and an identity-pose pair."""
    kinds = [{}, {}, {}, dict(cluster=True, held=0.35), dict(conflict=True), {}, dict(identity=True), {}]
    pairs = [random_pair(300 + f, p, n_cur=N_CUR[f], n_kf=N_KF[f], **kinds[f]) for f in range(8)]
    return [c for c, _, _ in pairs], [k for _, k, _ in pairs], np.stack([t for _, _, t in pairs])


MAIN = (3, 4, 6)      # the pairs of ragged_batch every non-vacuity condition holds for


# ==== the keyframe database and its query ========================================================================================================
def bow_of(V, desc):
    """(ascending words i32, values f64) of a frame: the BowVector of tests/bow_model.transform at levelsup 4."""
    from tests import bow_model as M
    bow = M.transform(V, desc, 4)[2]
    return np.array(list(bow), np.int32), np.array(list(bow.values()), np.float64)


def database_scene(seed, k=6, L=3, n_kf=60, n_query=5, n_desc=120):
    """A vocabulary (tests/bow_scenes.full_vocab, L1), n_kf keyframe BowVectors, a covisibility table and n_query consecutive query
    frames.  Keyframes come in groups of five that share most of their descriptors (covisible views of one place: several keyframes pass
    the 0.8 word threshold, their neighbours accumulate, a strong member is the pBestKF of its neighbours); every query mixes the
    descriptors of one group, of a second group and noise (the other groups share words but are not scored).  covis rows: the last two
    members of a group list the group, every row ends in a few random slots.  Returns (vocab args, V, keyframes [(words, values)], covis, queries [dict bow_word,
    bow_value])."""
    from tests import bow_model as M
    from tests import bow_scenes as S
    rng = np.random.Generator(np.random.PCG64(seed))
    args = S.full_vocab(seed, k=k, L=L, p_zero=0.0)
    V = M.build(*args)
    groups = (n_kf + 4) // 5
    base = [S.frame_descs(seed * 100 + g, args, n_desc) for g in range(groups)]
    kfs, descs = [], []
    for s in range(n_kf):
        d = base[s // 5].copy()
        drop = rng.random(n_desc) < 0.25 * (s % 5) / 4                    # later members of a group see less of it
        d[drop] = S.frame_descs(seed * 1000 + s, args, n_desc)[drop]
        descs.append(d)
        kfs.append(bow_of(V, d))
    covis = []
    for s in range(n_kf):
        g = s // 5
        row = [t for t in range(5 * g, min(5 * g + 5, n_kf)) if t != s]
        rng.shuffle(row)
        row = row if s % 5 >= 3 else []                                   # two members per group list their group (their pBestKF is shared: de-duplication)
        row += [int(x) for x in rng.integers(0, n_kf, 3)]
        covis.append(row[:10])
    queries = []
    for q in range(n_query):
        g1, g2 = (q * 3) % groups, (q * 3 + 1) % groups
        d = np.concatenate([base[g1][rng.random(n_desc) < 0.8], base[g2][rng.random(n_desc) < 0.75], S.frame_descs(seed * 77 + q, args, 20)])
        w, v = bow_of(V, d)
        queries.append(dict(bow_word=w, bow_value=v))
    return args, V, kfs, covis, queries


# The main scenes: every query of them meets the non-vacuity conditions of tests/test_reloc_model.py (small vocabularies, so that
# several keyframes pass the 0.8 word threshold and several accumulated scores pass 0.75 of the best).
MAIN_DATABASE_SCENES = [dict(seed=21, k=3, L=4, n_kf=40, n_desc=60), dict(seed=20, k=4, L=3, n_kf=50, n_desc=60)]
# Further shapes for parity only (wide vocabularies, up to 200 keyframes: one place wins clearly, so few candidates are retained there).
DATABASE_SCENES = MAIN_DATABASE_SCENES + [dict(seed=12, k=6, L=3, n_kf=60), dict(seed=13, k=10, L=3, n_kf=200, n_desc=60)]

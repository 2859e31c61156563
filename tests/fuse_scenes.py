"""Fixed-seed keyframe graphs for msl_fuse_map_points / msl_fuse_candidates: ten keyframes of about 150 keypoints at 160 x 120-scale
intrinsics (grid cells of 2.5 pixels, so a window can hold more than 64 cells) around about 90 world points.  A world point has a keypoint
in most keyframes that see it and up to three map points: an old one held by some target keyframes, a new one held by the current keyframe
(its duplicate), or three rivals held by different targets.  Some held points are bad, some normals look away, some distance ranges are
short, one keyframe looks backwards; one point projects into the corner of the current keyframe's image and one keypoint of the current
keyframe has a twin with the same descriptor one cell to its left.
graph(name) -> a fresh fuse_model.Graph with (prm, cur, targets); runs(name) -> the literal function's and the replay's results and every
batched call the replay made, computed once and shared.  Seeds are chosen so that tests/test_fuse_model.py::test_margins holds."""
import functools
import math

import numpy as np

from tests import fuse_model as fm
from tests.triangulate_scenes import KP, desc_flip, make_pose

F32 = np.float32
FX, FY, CX, CY, BF = 100.0, 100.0, 79.5, 59.5, 8.0
W, H = 160.0, 120.0
N_KF, CUR, TARGETS = 10, 0, (3, 1, 7, 2, 5, 4, 6)                        # 7 looks backwards; 8 and 9 only hold observations
SEEDS = dict(a=206, b=212, c=224)
ALL = tuple(SEEDS)


def prm(**kw):
    return fm.params(FX, FY, CX, CY, BF, 0.0, W, 0.0, H, **kw)


def grid_cell(x, y):
    """Frame::PosInGrid (src/Frame.cc:383-394) as the cell index ix * 48 + iy, -1 outside the grid."""
    px = int(np.round(F32(x) * (F32(64) / F32(W)))); py = int(np.round(F32(y) * (F32(48) / F32(H))))
    return px * 48 + py if 0 <= px < 64 and 0 <= py < 48 else -1


def _project(T, X):
    Xc = T[:, :3].astype(float) @ np.asarray(X, float) + T[:, 3].astype(float)
    return FX * Xc[0] / Xc[2] + CX, FY * Xc[1] / Xc[2] + CY, Xc[2]


def _centre(T):
    return -T[:, :3].astype(float).T @ T[:, 3].astype(float)


def _build(seed):
    r = np.random.RandomState(seed)
    sf = prm()["scale_factors"].astype(float)
    poses = []
    for k in range(N_KF):
        c = (r.uniform(-0.7, 0.7), r.uniform(-0.15, 0.15), r.uniform(-0.4, 0.4))
        rv = r.uniform(-0.08, 0.08, 3)
        if k == 7:
            rv = np.array([0.0, math.pi, 0.0]) + r.uniform(-0.05, 0.05, 3)
        poses.append(make_pose(c, rv))
    poses[CUR] = make_pose((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    feats = [[] for _ in range(N_KF)]

    def add_kp(k, u, v, octave, stereo, z, desc):
        feats[k].append(dict(x=F32(u), y=F32(v), octave=int(octave), ur=F32(u - BF / z) if stereo else F32(-1), desc=desc))
        return len(feats[k]) - 1

    M = 90
    z = r.uniform(2.0, 6.0, M)
    world = np.stack([r.uniform(-0.75, 0.75, M) * z, r.uniform(-0.55, 0.55, M) * z, z], 1)
    # the corner point: projects to (1.2, 1.3) of the current keyframe
    world[0] = [(1.2 - CX) / FX * 3.0, (1.3 - CY) / FY * 3.0, 3.0]
    plan = []                                                              # per world point: (kind, {kf: keypoint index})
    for w in range(M):
        X = world[w]
        base = r.randint(0, 256, 32).astype(np.uint8)
        D = np.linalg.norm(X - _centre(poses[CUR])) * 1.2 ** r.randint(0, 7) * r.uniform(1.02, 1.15)
        kind = "abcde"[int(np.searchsorted([0.3, 0.65, 0.78, 0.88], r.uniform()))]
        if w == 0:
            kind = "a"
        if w == 1:
            kind = "t"                                                     # the twin keypoints, a kind-a point otherwise
        seen = {}
        for k in range(N_KF):
            u, v, zc = _project(poses[k], X)
            if zc <= 0.3 or not (0.8 <= u < W - 2.5 and 0.8 <= v < H - 2.5):
                continue
            if r.uniform() > (0.85 if w > 1 else 1.0):
                continue
            d = np.linalg.norm(X - _centre(poses[k]))
            o = min(max(int(math.ceil(math.log(D / d) / math.log(1.2))), 0), 7)
            if o >= 1 and r.uniform() < 0.25:
                o -= 1
            if kind == "t":
                o = 1                                                      # every view at octave 1: the predicted level is 1 or 2
            noise = (0.45 if r.uniform() < 0.8 else 1.6) * sf[o] if w > 1 else 0.0
            du, dv = r.normal(0, noise), r.normal(0, noise)
            if kind == "t" and k == CUR:                                   # the twins: 2.8 pixels apart, the right one first
                du, dv = 1.4, 0.0
            stereo = r.uniform() < 0.5 and kind != "t"
            seen[k] = add_kp(k, u + du, v + dv, o, stereo, zc * (1 + r.normal(0, 0.01)), desc_flip(base, r, r.randint(0, 7)))
        plan.append((kind, seen, base))
    for k in range(N_KF):                                                  # clutter
        for _ in range(45):
            add_kp(k, r.uniform(0, W), r.uniform(0, H), r.randint(0, 8), r.uniform() < 0.5, r.uniform(1, 6), r.randint(0, 256, 32).astype(np.uint8))
    kind, seen, base = plan[1]
    if CUR in seen:                                                        # the left twin: the later index, the earlier cell
        f = feats[CUR][seen[CUR]]
        feats[CUR].append(dict(f, x=F32(float(f["x"]) - 2.8), desc=f["desc"].copy()))
    data = []
    for k in range(N_KF):
        fl = feats[k]
        kp = np.zeros(len(fl), KP)
        kp["x"] = [f["x"] for f in fl]; kp["y"] = [f["y"] for f in fl]; kp["size"] = 31.0; kp["octave"] = [f["octave"] for f in fl]; kp["class_id"] = -1
        data.append(dict(kps_un=kp, uright=np.array([f["ur"] for f in fl], F32), grid_cell=np.array([grid_cell(f["x"], f["y"]) for f in fl], np.int32),
                         desc=np.array([f["desc"] for f in fl], np.uint8).reshape(len(fl), 32), Tcw=poses[k]))
    g = fm.Graph(data)

    def point(w, kfs, look_away=False, short=False):
        X = world[w] + r.normal(0, 0.004, 3)
        n = np.zeros(3)
        for k in kfs:
            v = X - _centre(poses[k]); n += v / np.linalg.norm(v)
        n /= len(kfs)
        if look_away:
            n = np.array([n[2], n[1], -n[0]]) * 0.9                        # a quarter turn about y
        ref = kfs[0]
        dmax = np.linalg.norm(X - _centre(poses[ref])) * sf[int(data[ref]["kps_un"]["octave"][plan[w][1][ref]])]
        if short:
            dmax *= 0.3
        mp = g.new_point(X, n, (dmax / sf[7], dmax))
        for k in kfs:
            g.observe(mp, k, plan[w][1][k])
        return mp

    def some(ks, lo, hi):
        ks = list(ks)
        if not ks:
            return []
        n = min(len(ks), r.randint(lo, hi + 1))
        return [ks[i] for i in r.permutation(len(ks))[:n]]

    for w, (kind, seen, base) in enumerate(plan):
        others = [k for k in seen if k != CUR]
        odd = r.uniform()
        flags = dict(look_away=odd < 0.05, short=0.05 <= odd < 0.1)
        if kind in "at":
            ks = some(others, 2, 5)
            if ks:
                point(w, ks, **(flags if w > 1 else {}))
        elif kind == "b":
            ka = some(others, 1, 5)
            if ka:
                point(w, ka)
            if CUR in seen:
                point(w, [CUR] + some([k for k in others if k not in ka], 0, 2), **flags)
        elif kind == "c":
            tg = [k for k in others if k in TARGETS]
            perm = [tg[i] for i in r.permutation(len(tg))]
            for part in (perm[0:1], perm[1:2], perm[2:4]):
                if part:
                    point(w, part)
        elif kind == "d":
            if CUR in seen:
                point(w, [CUR] + some(others, 0, 1), **flags)
        else:
            ka = some(others, 1, 3)
            if ka:
                point(w, ka).bad = True                                    # bad, and still in its slots
            if CUR in seen:
                point(w, [CUR] + some([k for k in others if k not in ka], 0, 1))
    for mp in g.mps:
        bad, mp.bad = mp.bad, False
        mp.compute_distinctive_descriptors()
        mp.bad = bad
    # a bad point and an empty slot in the current keyframe's own list are part of every graph: kind e gives bad holders in targets; here
    # one of the current keyframe's points turns bad in place
    mine = [s for s in g.kfs[CUR].slots if s is not None]
    if mine:
        mine[len(mine) // 2].bad = True
    return g


def graph(name):
    """A fresh graph (the functions under test change it) and (prm, cur, targets)."""
    return _build(SEEDS[name]), prm(), CUR, list(TARGETS)


@functools.lru_cache(maxsize=None)
def runs(name):
    """dict(literal = (rets, snapshot), replay = (rets, stats, snapshot), calls = every batched fuse call of the replay as (table, points,
    items, lists, results), cand = the candidate call as (table, points, items, result))."""
    g, p, cur, targets = graph(name)
    rets = fm.search_in_neighbors_literal(g, p, cur, targets)
    lit = (rets, g.snapshot())
    g, p, cur, targets = graph(name)
    entry = fm.ModelEntry()
    cand = {}
    plain = entry.candidates

    def candidates(table, points, items):
        cand["call"] = (table, points, items, fm.fuse_candidates(table, points, items))
        return plain(table, points, items)
    entry.candidates = candidates
    rets, stats = fm.replay(g, p, cur, targets, entry)
    return dict(literal=lit, replay=(rets, stats, g.snapshot()), calls=entry.calls, cand=cand["call"])


@functools.lru_cache(maxsize=None)
def margins(name):
    """Every comparison of the two large batched calls of runs(name), as (what, lhs, rhs, scale)."""
    m = []
    for table, points, items, lists, _ in runs(name)["calls"]:
        if len(lists[0]) > 1:
            fm.fuse_map_points(prm(), table, points, items, lists, margins=m)
    return m

"""Fixed-seed keyframe graphs for msl_fuse_map_lines / msl_refresh_map_lines: ten keyframes in a box room (6 x 4 x 6 m) at 320 x 240-scale
intrinsics, about 34 3-D segments on its walls, each seen by 6 to 10 keyframes; at most 40 keylines per keyframe as in the reference, plus
one target keyframe filled with clutter to 256.  A segment has a keyline in most keyframes that see it and up to three map lines: an old
one held by some target keyframes, a new one held by the current keyframe and some targets (its duplicate; where a target holds it at the
best keyline that is the self-hit), or three rivals held by different targets (several hits on one slot of the current keyframe).  Some
keyframes have a second, empty keyline on a segment whose descriptor is closer to the line's than the slot that holds it (the add of a line
that is already in the keyframe); some held lines are bad, some normals look away, some distance ranges are short, some keylines have a
foreign descriptor or an octave outside the window; keyframe 7 looks backwards; the current keyframe holds one line in two slots.
graph(name) -> a fresh linefuse_model.Graph with (prm, cur, targets); runs(name) -> the literal function's and the replay's results and
every batched call the replay made, computed once and shared.  Seeds are chosen so that tests/test_linefuse_model.py::test_margins holds."""
import functools
import math

import numpy as np

from manhattanslam_amd import KEYLINE_DTYPE
from tests import linefuse_model as lf
from tests.triangulate_scenes import desc_flip, make_pose

F32 = np.float32
FX, FY, CX, CY = 200.0, 200.0, 159.5, 119.5
W, H = 320.0, 240.0
N_KF, CUR, TARGETS, BIG = 10, 0, (3, 1, 7, 2, 5, 4, 6), 6                 # 7 looks backwards; 8 and 9 only hold observations; 6 has 256 keylines
SEEDS = dict(a=33, b=66, c=72)
ALL = tuple(SEEDS)


def prm(**kw):
    return lf.params(FX, FY, CX, CY, 0.0, W, 0.0, H, **kw)


def _project(T, X):
    Xc = T[:, :3].astype(float) @ np.asarray(X, float) + T[:, 3].astype(float)
    return FX * Xc[0] / Xc[2] + CX, FY * Xc[1] / Xc[2] + CY, Xc[2]


def _centre(T):
    return -T[:, :3].astype(float).T @ T[:, 3].astype(float)


def _segment(r):
    """A segment of 0.3 to 0.9 m on the front wall (z = 5) or a side wall (x = +-3, z in 3.2 .. 5)."""
    wall = r.randint(0, 4)
    if wall < 2:
        a = np.array([r.uniform(-2.6, 2.6), r.uniform(-1.7, 1.7), 5.0])
        d = np.array([r.uniform(-1, 1), r.uniform(-1, 1), 0.0])
    else:
        a = np.array([3.0 if wall == 2 else -3.0, r.uniform(-1.7, 1.7), r.uniform(3.4, 4.8)])
        d = np.array([0.0, r.uniform(-1, 1), r.uniform(-1, 1)])
    d = d / np.linalg.norm(d) * r.uniform(0.3, 0.9)
    return np.concatenate([a - 0.5 * d, a + 0.5 * d])


def _build(seed):
    r = np.random.RandomState(seed)
    sf = prm()["scale_factors"].astype(float)
    poses = []
    for k in range(N_KF):
        c = (r.uniform(-0.8, 0.8), r.uniform(-0.3, 0.3), r.uniform(-0.5, 0.5))
        rv = r.uniform(-0.06, 0.06, 3)
        if k == 7:
            rv = np.array([0.0, math.pi, 0.0]) + r.uniform(-0.05, 0.05, 3)
        poses.append(make_pose(c, rv))
    poses[CUR] = make_pose((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    feats = [[] for _ in range(N_KF)]

    def add_kl(k, x, y, angle, octave, desc):
        feats[k].append(dict(x=F32(x), y=F32(y), angle=F32(angle), octave=int(octave), desc=desc))
        return len(feats[k]) - 1

    M = 34
    world = np.stack([_segment(r) for _ in range(M)])
    plan = []                                                              # per segment: (kind, {kf: keyline index}, {kf: twin keyline index})
    for w in range(M):
        P = world[w]
        mid = 0.5 * (P[:3] + P[3:])
        base = r.randint(0, 256, 32).astype(np.uint8)
        D = np.linalg.norm(mid - _centre(poses[CUR])) * 1.2 ** r.randint(0, 7) * r.uniform(1.02, 1.15)
        kind = "abcde"[int(np.searchsorted([0.25, 0.65, 0.8, 0.88], r.uniform()))]
        seen, twin = {}, {}
        for k in range(N_KF):
            u1, v1, z1 = _project(poses[k], P[:3]); u2, v2, z2 = _project(poses[k], P[3:])
            if min(z1, z2) <= 0.3 or not all(2.0 <= u < W - 2.0 for u in (u1, u2)) or not all(2.0 <= v < H - 2.0 for v in (v1, v2)):
                continue
            if abs(u1 - u2) < 0.5 or r.uniform() > 0.9:
                continue
            d = np.linalg.norm(mid - _centre(poses[k]))
            o = min(max(int(math.ceil(math.log(D / d) / math.log(1.2))), 0), 7)
            if o >= 1 and r.uniform() < 0.25:
                o -= 1
            odd = r.uniform()
            if odd < 0.06:
                o = (o + 3) % 8                                            # an octave outside the window
            noise = 0.4 * sf[o]
            slope = (v1 - v2) / (u1 - u2)
            angle = slope + (r.uniform(0.05, 0.6) if odd > 0.12 else -r.uniform(0.3, 0.9))   # GetLinesInArea keeps slope - angle <= 0.01 r
            desc = desc_flip(base, r, r.randint(1, 9)) if not 0.12 < odd < 0.2 else r.randint(0, 256, 32).astype(np.uint8)
            x, y = 0.5 * (u1 + u2) + r.normal(0, noise), 0.5 * (v1 + v2) + r.normal(0, noise)
            seen[k] = add_kl(k, x, y, angle, o, desc)
            if r.uniform() < 0.12 and len(feats[k]) < 38:                  # an empty twin whose descriptor is the segment's own
                twin[k] = add_kl(k, x + r.normal(0, 0.3), y + r.normal(0, 0.3), angle, o, base.copy())
        plan.append((kind, seen, twin))
    for k in range(N_KF):                                                  # clutter, the big keyframe to 256
        for _ in range((256 if k == BIG else min(40, len(feats[k]) + 4)) - len(feats[k])):
            add_kl(k, r.uniform(0, W), r.uniform(0, H), r.uniform(-1.5, 1.5), r.randint(0, 8), r.randint(0, 256, 32).astype(np.uint8))
    data = []
    for k in range(N_KF):
        fl = feats[k]
        kl = np.zeros(len(fl), KEYLINE_DTYPE)
        kl["x"] = [f["x"] for f in fl]; kl["y"] = [f["y"] for f in fl]; kl["angle"] = [f["angle"] for f in fl]; kl["octave"] = [f["octave"] for f in fl]
        data.append(dict(kl=kl, ldesc=np.array([f["desc"] for f in fl], np.uint8).reshape(len(fl), 32), Tcw=poses[k]))
    g = lf.Graph(data)

    def line(w, kfs, look_away=False, short=False):
        P = np.round((world[w] + r.normal(0, 0.003, 6)) * 4096.0) / 4096.0   # exact in float, and so is the midpoint
        mid = 0.5 * (P[:3] + P[3:])
        n = np.zeros(3)
        for k in kfs:
            v = mid - _centre(poses[k]); n += v / np.linalg.norm(v)
        n /= len(kfs)
        if look_away:
            n = np.array([n[2], n[1], -n[0]]) * 0.9                        # a quarter turn about y
        ref = kfs[0]
        # a little below dist * scale: in the reference keyframe itself log(ratio) / logScale would sit on the integer that ceil rounds to
        dmax = np.linalg.norm(mid - _centre(poses[ref])) * sf[int(data[ref]["kl"]["octave"][plan[w][1][ref]])] * r.uniform(0.93, 0.98)
        if short:
            dmax *= 0.3
        ml = g.new_line(P, n, (dmax / sf[7], dmax), ref)
        for k in kfs:
            g.observe(ml, k, plan[w][1][k])
        return ml

    def some(ks, lo, hi):
        ks = list(ks)
        if not ks:
            return []
        n = min(len(ks), r.randint(lo, hi + 1))
        return [ks[i] for i in r.permutation(len(ks))[:n]]

    for w, (kind, seen, twin) in enumerate(plan):
        others = [k for k in seen if k != CUR]
        odd = r.uniform()
        flags = dict(look_away=odd < 0.05, short=0.05 <= odd < 0.1)
        if kind == "a":
            ks = some(others, 2, 5)
            if ks:
                line(w, ks, **flags)
        elif kind == "b":
            ka = some(others, 1, 4)
            if ka:
                line(w, ka)
            if CUR in seen:
                line(w, [CUR] + some([k for k in others if k not in ka], 0, 3), **flags)
        elif kind == "c":
            tg = [k for k in others if k in TARGETS]
            perm = [tg[i] for i in r.permutation(len(tg))]
            for part in (perm[0:1], perm[1:2], perm[2:4]):
                if part:
                    line(w, part)
        elif kind == "d":
            if CUR in seen:
                line(w, [CUR] + some(others, 0, 3), **flags)
        else:
            ka = some(others, 1, 3)
            if ka:
                line(w, ka).bad = True                                     # bad, and still in its slots
            if CUR in seen:
                line(w, [CUR] + some([k for k in others if k not in ka], 0, 2))
    for ml in g.mls:
        bad, ml.bad = ml.bad, False
        ml.compute_distinctive_descriptors()
        ml.bad = bad
    mine = [s for s in g.kfs[CUR].slots if s is not None]
    if mine:
        mine[len(mine) // 2].bad = True                                    # a bad line in the current keyframe's own list
    # the current keyframe holds one line in two slots (what an earlier add of a line already in the keyframe leaves)
    free = [i for i, s in enumerate(g.kfs[CUR].slots) if s is None]
    good = [s for s in mine if not s.bad]
    if free and good:
        g.kfs[CUR].slots[free[-1]] = good[0]
    return g


def graph(name):
    """A fresh graph (the functions under test change it) and (prm, cur, targets)."""
    return _build(SEEDS[name]), prm(), CUR, list(TARGETS)


@functools.lru_cache(maxsize=None)
def runs(name):
    """dict(literal = (rets, snapshot), replay = (rets, stats, snapshot), calls = every batched fuse call of the replay as (table, lines,
    items, lists, results), cand = the candidate call as (table, lines, items, result), entry = the state before anything ran)."""
    g, p, cur, targets = graph(name)
    entry_state = (g.table(), g.lines(), [ml.observations() for ml in g.mls])
    rets = lf.search_in_neighbors_lines_literal(g, p, cur, targets)
    lit = (rets, g.snapshot())
    g, p, cur, targets = graph(name)
    entry = lf.ModelEntry()
    cand = {}
    plain = entry.candidates

    def candidates(table, lines, items):
        cand["call"] = (table, lines, items, lf.fuse_candidates(table, lines, items))
        return plain(table, lines, items)
    entry.candidates = candidates
    rets, stats = lf.replay(g, p, cur, targets, entry)
    return dict(literal=lit, replay=(rets, stats, g.snapshot()), calls=entry.calls, cand=cand["call"], entry=entry_state)


@functools.lru_cache(maxsize=None)
def margins(name):
    """Every comparison of the two large batched calls of runs(name), as (what, lhs, rhs, scale)."""
    m = []
    for table, lines, items, lists, _ in runs(name)["calls"]:
        if len(lists[0]) > 1:
            lf.fuse_map_lines(prm(), table, lines, items, lists, margins=m)
    return m

"""Scenes for the LocalMapping search and fusion entries at the limits include/msl.h accepts: cap 8192, n_tab 4096, n_pts / n_lines 1 << 20,
lcap 65536, tcap 64, klcap 256, ccap = n_tab and n_items 4096 (1 << 20 for the refresh).  One cached builder per case; each returns a dict
with the packed inputs `a` (keyed by msl.h's argument names), the shape `sh`, the expected outputs `e` of the sequential models
(tests/fuse_model.py, tests/linefuse_model.py, tests/mappoint_model.py, tests/triangulate_model.py) and the `facts` it was built to reach.
tests/test_search_limit_scenes.py asserts those facts without a GPU, tests/test_search_limits_gpu.py runs the entries on the same arrays.
Nobody changes what a builder returned.

  msl_fuse_candidates     C1  tcap 64 targets of cap 8192 slots, lcap 65536: n_cand above lcap and n_cand = lcap - 1
                          C2  n_pts 1 << 20 and 40 items: launches of 16, 16 and 8 items over one scratch buffer
                          C3  n_items 4096 in one launch, rows tiled with period 37
  msl_fuse_map_points     P1  one keyframe of 8192 keypoints, a list of 65536 entries, a point table of 1 << 20
                          P2  n_items = n_lists = n_tab = 4096, tiled with period 37
  msl_fuse_map_lines      L1  one keyframe of 256 keylines, a list of 65536 entries, a line table of 1 << 20
                          L2  n_items = n_lists = n_tab = 4096, tiled with period 37
  msl_triangulate_new_points  T1  ncap 16 with sixteen neighbours inside a table of 4096, the current keyframe at 4095
                          T2  n_items 65535 (the grid limit of the item dimension), cap 8, tiled with period 37
  msl_refresh_map_points  R1  n_pts 1 << 20, n_tab 4096 (cap 128): keyframe 4095, 256 and 257 live observations
                          R1c n_pts 1 << 20, cap 8192 (n_tab 8): keypoint index 8191
                          R2  n_items = n_pts = 1 << 20
  msl_refresh_map_lines   R3  n_lines 1 << 20, klcap 256, n_tab 4096
  msl_covisibility        V1  n_tab = ccap 4096, cap 8192: weight 8192, n_conn 4095
                          V2  n_items = n_tab 4096: weight is 4096 x 4096

Limits that are covered apart and not together:
  n_items 4096 and lcap 65536 (C1 / C3, P1 / P2, L1 / L2): an output array alone would have 1 GiB
  n_items 65535 and n_tab 4096 / ncap 16 of msl_triangulate_new_points (T1 / T2): T2 is about blockIdx.z alone
  n_items 4096 and n_pts 1 << 20 of msl_fuse_candidates (C2 / C3): C2 is about the launches that n_pts splits, C3 about one launch
  n_tab 4096 and cap 8192 of msl_refresh_map_points (R1 / R1c): the keypoint and descriptor tables would have 2 GiB; so the reference
    keyframe 4095 has reference index 127 in R1, and reference index 8191 belongs to keyframe 7 in R1c
  n_items 4096 and cap 8192 of msl_covisibility (V1 / V2), and V2's ccap is 16: conn and conn_w at ccap 4096 would add 128 MB
A tiled case runs the model on its distinct elements only and tiles the expectation.
The margin rule of tests/test_fuse_model.py::test_margins holds in every searching case.  P1, P2, L1 and L2 get there by retiring the
candidates that have a comparison within 1e-3 of its threshold: the point or line turns bad, leaves at the second exit and keeps its place
in the list; `facts` counts them (at most 5 % of the live ones).  T1 and T2 get there by their seeds alone."""
import functools

import numpy as np

from tests import fuse_model as fm
from tests import fuse_scenes as fs
from tests import linefuse_model as lf
from tests import linefuse_scenes as ls
from tests import mappoint_model as mm
from tests import triangulate_model as tm
from tests import triangulate_scenes as ts
from tests.localmap_scenes import FILL
from tests.triangulate_scenes import KP, make_pose

F32 = np.float32
MAX_CAP, MAX_TAB, MAX_PTS, MAX_LCAP, MAX_TCAP, MAX_ITEMS, MAX_KLCAP = 8192, 4096, 1 << 20, 65536, 64, 4096, 256
CAND_SCRATCH = 1 << 24                                                 # entries the items of one k_fuse_cand launch share
PERIOD = 37                                                            # of the tiled cases: divides neither 4096 nor 65535
MARGIN, RETIRED_CAP = 1e-3, 0.05


def filled(shape, dtype):
    """An array whose every byte is FILL: what an output holds before the call."""
    return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, FILL, np.uint8).view(dtype).reshape(shape)


def tile(rows, n):
    """rows repeated along the first axis to n rows."""
    return np.ascontiguousarray(np.resize(rows, (n,) + rows.shape[1:]))


def _first_seen(table, flags, targets):
    """The candidate list by numpy: (ids in order, their positions rank * cap + slot).  Only used to shape a scene; the expectation is the
    model's."""
    cap = len(table[0]["held_id"])
    flat = np.concatenate([table[t]["held_id"] for t in targets])
    pos = np.flatnonzero((flat >= 0) & (flags[np.clip(flat, 0, len(flags) - 1)] == 1))
    ids, first = np.unique(flat[pos], return_index=True)
    order = np.sort(first)
    assert cap * len(targets) == len(flat)
    return flat[pos][order], pos[order]


# ---- msl_fuse_candidates ---------------------------------------------------------------------------------------------------------------
def _cand_case(table, flags, items, tcap, lcap, facts, tiled=None):
    """Packed inputs and the model's lists.  tiled: n_items, the items given being one period."""
    from manhattanslam_amd._lib import pad
    cap = max(len(k["held_id"]) for k in table)
    want = fm.fuse_candidates(table, dict(flags=flags), items, lcap=lcap)
    F = len(items)
    targets = np.full((F, tcap), -1, np.int32)
    for f, it in enumerate(items):
        targets[f, :len(it)] = it
    n_targets = np.array([len(i) for i in items], np.int32)
    cand = np.full((F, lcap), -1, np.int32)
    for f, (lst, _) in enumerate(want):
        cand[f, :len(lst)] = lst
    n_cand = np.array([n for _, n in want], np.int32)
    if tiled:
        targets, n_targets, cand, n_cand, F = tile(targets, tiled), tile(n_targets, tiled), tile(cand, tiled), tile(n_cand, tiled), tiled
    a = dict(held_id=pad(table, "held_id", cap, np.int32, fill=-1), n_kps=np.array([len(k["held_id"]) for k in table], np.int32),
             pt_flags=flags, targets=targets, n_targets=n_targets)
    sh = dict(n_tab=len(table), cap=cap, n_pts=len(flags), n_items=F, tcap=tcap, lcap=lcap)
    return dict(a=a, sh=sh, e=dict(cand=cand, n_cand=n_cand), facts=facts, items=items, want=want)


@functools.lru_cache(maxsize=None)
def c1():
    """C1.  66 keyframes of 8192 slots over a point table of 1 << 20.  Item 0 names 64 targets, keyframe 5 twice: more than 65536 distinct
    live ids.  `both` sits in rank 0 slot 8191 and in rank 63 slot 0, `twice` in two slots of rank 0, ids 0 and 1048575 in rank 0.  Item 1
    names twelve keyframes that hold exactly lcap - 1 distinct live ids."""
    rng = np.random.default_rng(101)
    n_tab, cap, n_pts, lcap = 66, MAX_CAP, MAX_PTS, MAX_LCAP
    flags = (rng.random(n_pts) > 0.1).astype(np.uint8)
    held = rng.integers(0, n_pts, (n_tab, cap)).astype(np.int32)
    held[rng.random((n_tab, cap)) < 0.2] = -1
    item0 = [3, 5] + [k for k in range(6, 57)] + [0, 1, 2, 4, 57, 58, 59, 60, 61, 5, 62]
    assert len(item0) == MAX_TCAP and len(set(item0)) == MAX_TCAP - 1
    first, last = item0[0], item0[-1]
    both, twice = 777777, 555555
    held[held == both] = -1; held[held == twice] = -1; held[(held == 0) | (held == n_pts - 1)] = -1
    flags[[both, twice, 0, n_pts - 1]] = 1
    held[first, cap - 1] = both; held[last, 0] = both
    held[first, 10] = held[first, 4000] = twice
    held[first, 0], held[first, 1] = n_pts - 1, 0
    bad_held = int(held[first, 2]) if held[first, 2] >= 0 else int(held[first][held[first] >= 0][5])
    flags[bad_held] = 0
    item1 = list(range(54, 66))
    table = [dict(held_id=held[k]) for k in range(n_tab)]
    ids, pos = _first_seen(table, flags, item1)
    assert len(ids) > lcap - 1
    surplus = set(ids[lcap - 1:].tolist())                            # the surplus ids leave these keyframes, every copy of theirs
    for k in item1:
        held[k][np.isin(held[k], list(surplus))] = -1
    table = [dict(held_id=held[k]) for k in range(n_tab)]
    facts = dict(both=both, twice=twice, bad_held=bad_held, first=first, last=last, ends=(0, n_pts - 1))
    return _cand_case(table, flags, [item0, item1], MAX_TCAP, lcap, facts)


@functools.lru_cache(maxsize=None)
def c2():
    """C2.  n_pts 1 << 20, so a launch takes CAND_SCRATCH / n_pts = 16 items and the 40 items go in launches of 16, 16 and 8: item f + 16
    and item f + 32 work in the scratch row item f used.  Item f < 16 names keyframe f alone; item f + 16 names 16 + f and then f; item
    f + 32 names 16 + f, 32 + f and then f.  So every live id of keyframe f, ids 0 and 1048575 among them, stands at a larger position in
    the later items."""
    rng = np.random.default_rng(102)
    n_tab, cap, n_pts = 48, 32, MAX_PTS
    flags = (rng.random(n_pts) > 0.1).astype(np.uint8)
    flags[[0, n_pts - 1]] = 1
    held = rng.integers(0, n_pts, (n_tab, cap)).astype(np.int32)
    held[rng.random((n_tab, cap)) < 0.15] = -1
    held[(held == 0) | (held == n_pts - 1)] = -1
    for f in range(16):
        held[f, 3], held[f, cap - 1] = 0, n_pts - 1
    items = [[f] for f in range(16)] + [[16 + f, f] for f in range(16)] + [[16 + f, 32 + f, f] for f in range(8)]
    table = [dict(held_id=held[k]) for k in range(n_tab)]
    return _cand_case(table, flags, items, 4, 128, dict(per_launch=CAND_SCRATCH // n_pts, ends=(0, n_pts - 1)))


@functools.lru_cache(maxsize=None)
def c3():
    """C3.  4096 items in one launch: 37 distinct rows of up to three targets over 41 keyframes of 8 slots and 500 points, tiled; lcap 12
    is less than some rows' counts."""
    rng = np.random.default_rng(103)
    n_tab, cap, n_pts = 41, 8, 500
    flags = (rng.random(n_pts) > 0.1).astype(np.uint8)
    table = []
    for k in range(n_tab):
        h = rng.integers(0, n_pts, int(rng.integers(0, cap + 1))).astype(np.int32)
        h[rng.random(len(h)) < 0.15] = -1
        table.append(dict(held_id=np.concatenate([h, np.full(cap - len(h), -1, np.int32)])[:cap]))
    items = [[int(k) for k in rng.permutation(n_tab)[:int(rng.integers(0, 4))]] for _ in range(PERIOD)]
    items[PERIOD - 1] = [n_tab - 1, 0, n_tab - 1]
    return _cand_case(table, flags, items, 3, 12, dict(period=PERIOD), tiled=MAX_ITEMS)


# ---- msl_covisibility ------------------------------------------------------------------------------------------------------------------
def _csr(obs_lists, n_pts):
    """obs_off / obs_kf / obs_idx from {point id: [(keyframe, keypoint)]}; every other point has an empty range."""
    cnt = np.zeros(n_pts, np.int64)
    for p, o in obs_lists.items():
        cnt[p] = len(o)
    off = np.zeros(n_pts + 1, np.int32)
    off[1:] = np.cumsum(cnt)
    flat = np.array([x for p in sorted(obs_lists) for x in obs_lists[p]], np.int32).reshape(-1, 2)
    if not len(flat):
        flat = np.zeros((1, 2), np.int32)
    return dict(obs_off=off, obs_kf=np.ascontiguousarray(flat[:, 0]), obs_idx=np.ascontiguousarray(flat[:, 1]))


class _Obs:
    """observations[id] of a model over a large table: the lists of the named points, () for every other."""

    def __init__(self, lists, n):
        self.lists, self.n = lists, n

    def __len__(self):
        return self.n

    def __getitem__(self, p):
        return self.lists.get(int(p), ())


@functools.lru_cache(maxsize=None)
def v1():
    """V1.  n_tab = ccap 4096, cap 8192.  Keyframe 7 holds 8192 live points, each observed by 7 itself and by keyframe 2000; every other
    keyframe observes 15 .. 20 of them (th 15), so n_conn is 4095, the weights below 8192 repeat, and the sort covers all of P = 4096."""
    rng = np.random.default_rng(104)
    n_tab, cap, k0, full = MAX_TAB, MAX_CAP, 7, 2000
    n_pts = cap + 8
    obs = {p: [(k0, p), (full, p)] for p in range(cap)}
    w = np.zeros(n_tab, np.int64)
    for j in range(n_tab):
        if j in (k0, full):
            continue
        w[j] = 15 + (j * 7) % 6
        for p in rng.choice(cap, int(w[j]), replace=False):
            obs[int(p)].append((j, 0))
    for p in obs:                                                     # the caller's order, not ascending
        o = obs[p]
        obs[p] = [o[i] for i in rng.permutation(len(o))]
    w[full] = cap
    flags = np.ones(n_pts, np.uint8); flags[cap:] = 0
    held = np.full((n_tab, cap), -1, np.int32)
    held[k0] = rng.permutation(cap)
    table = [dict(held_id=held[k0] if k == k0 else held[k][:0]) for k in range(n_tab)]
    e = mm.covisibility(table, _Obs(obs, n_pts), flags, [k0], th=15, ccap=n_tab)
    a = dict(held_id=held, n_kps=np.array([cap if k == k0 else 0 for k in range(n_tab)], np.int32), pt_flags=flags, kf=np.array([k0], np.int32),
             **{k: v for k, v in _csr(obs, n_pts).items() if k != "obs_idx"})
    sh = dict(n_tab=n_tab, cap=cap, n_pts=n_pts, n_items=1, n_obs_total=int(a["obs_off"][-1]), ccap=n_tab, th=15)
    return dict(a=a, sh=sh, e=e, facts=dict(item=k0, full=full, weights=w))


@functools.lru_cache(maxsize=None)
def v2():
    """V2.  n_items = n_tab 4096, cap 8, ccap 16, th 2.  Keyframe k holds row k % 37 of 37 distinct rows; the points of row r are observed
    by keyframes that are not r modulo 37, so the item's own index never matters and the model runs on items 0 .. 36.  Three keyframes
    (100, 2049 and 4095) hold rows of their own whose points they observe themselves; the model runs on those too."""
    rng = np.random.default_rng(105)
    n_tab, cap, n_pts = MAX_TAB, 8, 400
    own = (100, 2049, n_tab - 1)
    obs, rows = {}, []
    flags = (rng.random(n_pts) > 0.1).astype(np.uint8)
    for r in range(PERIOD):
        row = rng.integers(0, 300, int(rng.integers(0, cap + 1))).astype(np.int32)
        row[rng.random(len(row)) < 0.1] = -1
        rows.append(row)
    member = {}
    for r, row in enumerate(rows):
        for p in row[row >= 0]:
            member.setdefault(int(p), set()).add(r)
    pool = np.array([0, 1, 2, 5, 40, 41, 2048, 2049, 4000, 4094, 4095] + rng.integers(0, n_tab, 30).tolist())
    for p in range(300):
        ks = [int(k) for k in pool[rng.permutation(len(pool))[:int(rng.integers(1, 14))]] if int(k) % PERIOD not in member.get(p, ())]
        obs[p] = [(k, 0) for k in ks]
    held = np.full((n_tab, cap), -1, np.int32)
    n_kps = np.zeros(n_tab, np.int32)
    for k in range(n_tab):
        held[k, :len(rows[k % PERIOD])] = rows[k % PERIOD]; n_kps[k] = len(rows[k % PERIOD])
    for k in own:
        mine = 300 + 10 * own.index(k) + np.arange(cap, dtype=np.int32)
        held[k], n_kps[k] = mine, cap
        for i, p in enumerate(mine):
            flags[p] = 1
            obs[int(p)] = [(int(j), 0) for j in pool[:3 + i]] + [(k, i)]
    model_items = list(range(PERIOD)) + list(own)
    table = [dict(held_id=held[k, :n_kps[k]]) for k in range(n_tab)]
    small = mm.covisibility(table, _Obs(obs, n_pts), flags, model_items, th=2, ccap=16)
    e = {k: tile(v[:PERIOD], n_tab) for k, v in small.items()}
    for i, k in enumerate(own):
        for key in e:
            e[key][k] = small[key][PERIOD + i]
    a = dict(held_id=held, n_kps=n_kps, pt_flags=flags, kf=np.arange(n_tab, dtype=np.int32),
             **{k: v for k, v in _csr(obs, n_pts).items() if k != "obs_idx"})
    sh = dict(n_tab=n_tab, cap=cap, n_pts=n_pts, n_items=n_tab, n_obs_total=int(a["obs_off"][-1]), ccap=16, th=2)
    return dict(a=a, sh=sh, e=e, facts=dict(own=own, period=PERIOD, model_items=model_items, small=small))


# ---- msl_refresh_map_points ------------------------------------------------------------------------------------------------------------
def _refresh_case(seed, n_tab, cap, n_real, every_point=False):
    """n_pts 1 << 20 with n_real points that have observations (1 .. 12, the two end ids among them), one point with 256 and one with 257
    live observations, a few bad points and a few without observations among the items.  The last keyframe and the last keypoint index
    are observed, and are reference keyframe and reference index of the last id.  every_point: the items are all ids, in a shuffled
    order."""
    rng = np.random.default_rng(seed)
    n_pts = MAX_PTS
    prm = mm.params()
    kp = np.zeros((n_tab, cap), KP)
    kp["octave"] = rng.integers(0, 8, (n_tab, cap)); kp["size"] = 31.0; kp["class_id"] = -1
    desc = rng.integers(0, 256, (n_tab, cap, 32), dtype=np.uint8)
    bad_kf = {3}
    table = [dict(desc=desc[k], kps_un=kp[k], Tcw=make_pose(rng.uniform(-1, 1, 3) * (0.8, 0.3, 0.5), rng.uniform(-0.1, 0.1, 3)), bad=k in bad_kf)
             for k in range(n_tab)]
    real = np.unique(np.concatenate([[0, n_pts - 1], rng.integers(1, n_pts - 1, n_real)]))
    last_kf, last_idx = n_tab - 1, cap - 1
    obs = {}
    for p in real:
        n = int(rng.integers(1, 13))
        ks = rng.permutation(n_tab)[:min(n, n_tab)]
        obs[int(p)] = [(int(k), int(rng.integers(0, cap))) for k in ks]
    many = [int(real[len(real) // 3]), int(real[len(real) // 2])]
    pool = [k for k in range(n_tab) if k not in bad_kf]
    if n_tab >= 300:
        for p, n in zip(many, (256, 257)):
            obs[p] = [(int(k), int(rng.integers(0, cap))) for k in rng.permutation(pool)[:n]] + [(3, 1)]   # and one in a bad keyframe
    else:
        many = []
    obs[n_pts - 1] = [(0, 5), (last_kf, last_idx), (1, last_idx)]     # the last id: the range ends at n_obs_total
    obs[0] = [(last_kf, 0), (2, last_idx)]
    flags = np.zeros(n_pts, np.uint8)
    flags[real] = 1
    dead = np.unique(rng.integers(1, n_pts - 1, 40))
    dead = dead[~np.isin(dead, real)]
    empty = real[5:45:4]                                              # live, without observations
    empty = empty[~np.isin(empty, [0, n_pts - 1] + many)]
    for p in empty:
        obs[int(p)] = []
    xyz = np.zeros((n_pts, 3), F32)
    z = rng.uniform(2, 6, len(real))
    xyz[real] = np.stack([rng.uniform(-0.6, 0.6, len(real)) * z, rng.uniform(-0.4, 0.4, len(real)) * z, z], 1)
    ref = np.zeros(n_pts, np.int32)
    for p in real:
        o = obs[int(p)]
        ref[p] = o[int(rng.integers(0, len(o)))][0] if o and rng.random() < 0.8 else int(rng.integers(0, n_tab))
    ref[n_pts - 1] = last_kf
    points = dict(flags=flags, xyz=xyz, ref=ref)
    named = np.concatenate([real, dead]).astype(np.int32)
    named = named[rng.permutation(len(named))]
    want = mm.refresh_map_points(prm, table, _Obs({p: o for p, o in obs.items() if o}, n_pts), points, named, select=mm.select_descriptor_fast)
    if every_point:
        ids = rng.permutation(n_pts).astype(np.int32)
        where = np.empty(n_pts, np.int64); where[ids] = np.arange(n_pts)
        e = dict(out_desc=np.zeros((n_pts, 32), np.uint8), out_normal=np.zeros((n_pts, 3), F32), out_dist=np.zeros((n_pts, 2), F32),
                 best_obs=np.full(n_pts, -1, np.int32), best_median=np.zeros(n_pts, np.int32), status=np.full(n_pts, mm.BAD, np.uint8))
        for k in e:                                                   # by rule: every point not named above is bad
            e[k][where[named]] = want[k]
    else:
        ids, e = named, want
    rows = dict(pt_desc=filled((n_pts, 32), np.uint8), pt_normal=filled((n_pts, 3), F32), pt_dist=filled((n_pts, 2), F32))
    d, n = (want["status"] & mm.DESC_WRITTEN) != 0, (want["status"] & mm.NORMAL_WRITTEN) != 0
    rows["pt_desc"][named[d]] = want["out_desc"][d]
    rows["pt_normal"][named[n]] = want["out_normal"][n]; rows["pt_dist"][named[n]] = want["out_dist"][n]
    from manhattanslam_amd import mappoint
    _, t = mappoint.pack_table(table, cap)
    a = dict(t, **_csr({p: o for p, o in obs.items() if o}, n_pts), pt_xyz=xyz, pt_flags=flags, pt_ref=ref, ids=ids)
    sh = dict(n_tab=n_tab, cap=cap, n_pts=n_pts, n_items=len(ids), n_obs_total=int(a["obs_off"][-1]), what=3)
    assert not np.isnan(want["out_normal"]).any()
    facts = dict(named=named, want=want, obs=obs, many=many, dead=dead, empty=empty, last_kf=last_kf, last_idx=last_idx, prm=prm)
    return dict(a=a, sh=sh, e=dict(e, **rows), facts=facts)


@functools.lru_cache(maxsize=None)
def r1():
    return _refresh_case(106, MAX_TAB, 128, 3000)


@functools.lru_cache(maxsize=None)
def r1c():
    return _refresh_case(107, 8, MAX_CAP, 3000)


@functools.lru_cache(maxsize=None)
def r2():
    return _refresh_case(108, 40, 64, 3000, every_point=True)


# ---- msl_fuse_map_points ---------------------------------------------------------------------------------------------------------------
W, H = fs.W, fs.H
HOLE = (100.0, 130.0, 20.0, 50.0)                                      # no keypoint of P1's keyframe lies in x 100 .. 130, y 20 .. 50


def _flip(desc, rng, nbits):
    d = desc.copy()
    for b in rng.choice(256, int(nbits), replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def _keyframe(rng, n, T, hole=None):
    """n random keypoints on the 160 x 120 image of tests/fuse_scenes.py: random octaves, half of them stereo, random descriptors."""
    x, y = rng.uniform(0.5, W - 3, n), rng.uniform(0.5, H - 3, n)
    if hole:
        inside = (x >= hole[0]) & (x < hole[1]) & (y >= hole[2]) & (y < hole[3])
        x[inside] -= 60.0
    kp = np.zeros(n, KP)
    kp["x"], kp["y"], kp["size"], kp["octave"], kp["class_id"] = x, y, 31.0, rng.integers(0, 8, n), -1
    ur = np.where(rng.random(n) < 0.5, x - fs.BF / rng.uniform(2, 6, n), -1.0).astype(F32)
    return dict(kps_un=kp, uright=ur, desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), Tcw=T)


def _finish_keyframe(kf, held):
    kp = kf["kps_un"]
    kf["grid_cell"] = np.array([fs.grid_cell(a, b) for a, b in zip(kp["x"], kp["y"])], np.int32)
    kf["held_id"] = held
    return kf


def _world(T, u, v, z):
    """The world point that T projects to (u, v) at depth z, and its view vector from the camera centre."""
    R, t = T[:, :3].astype(float), T[:, 3].astype(float)
    Xc = np.array([(u - fs.CX) / fs.FX * z, (v - fs.CY) / fs.FY * z, z])
    X = R.T @ (Xc - t)
    return X, X + R.T @ t


def _seen_point(rng, pts, p, T, u, v, level, desc, look_away=False, short=False):
    """Point p of the table: projects to (u, v), its distance range predicts `level`, its normal looks at the camera."""
    X, view = _world(T, u, v, rng.uniform(2, 6))
    d = np.linalg.norm(view)
    dmax = d * 1.2 ** (level - rng.uniform(0.2, 0.8)) * (0.3 if short else 1.0)
    pts["xyz"][p], pts["normal"][p] = X, (-1 if look_away else 1) * view / d
    pts["dist"][p], pts["desc"][p] = (dmax / 1.2 ** 7, dmax), desc


def _retire(prm, kf, pts, live):
    """The margin rule: a live candidate with a comparison within MARGIN of its threshold turns bad and leaves at the second exit; its
    place in the list stays.  Returns the retired ids."""
    kf = dict(kf, _grid=fm.grid_of(kf))
    gone = []
    for p in live:
        m = []
        fm.search_one(prm, kf, pts["xyz"][p], pts["normal"][p], pts["dist"][p], pts["desc"][p], m, {})
        if any(abs(lhs - rhs) <= MARGIN * abs(scale) for _, lhs, rhs, scale in m):
            pts["flags"][p] = 0
            gone.append(int(p))
    return gone


def fuse_margins(prm, kf, pts, lst):
    """Every comparison of the candidates of lst that reach the search, as (what, lhs, rhs, scale)."""
    m = []
    fm.fuse_item(prm, kf, pts, lst, margins=m)
    return m


def _point_table(n_pts):
    return dict(xyz=np.zeros((n_pts, 3), F32), normal=np.zeros((n_pts, 3), F32), dist=np.zeros((n_pts, 2), F32), desc=np.zeros((n_pts, 32), np.uint8),
                flags=np.zeros(n_pts, np.uint8), nobs=np.zeros(n_pts, np.int32))


def _fuse_pack(table, pts, items, lists, cap, lcap, results):
    """Packed inputs of msl_fuse_map_points and the expected arrays from one fuse_item result per item."""
    from manhattanslam_amd import fuse
    _, t = fuse.pack_table(table, cap)
    n_pts, p = fuse.pack_points(pts)
    _, cand, n_cand = fuse.pack_lists(lists, lcap)
    F = len(items)
    e = dict(best_idx=np.full((F, lcap), -1, np.int32), best_dist=np.zeros((F, lcap), np.int32), status=np.zeros((F, lcap), np.uint8),
             other=np.full((F, lcap), -1, np.int32), n_fused=np.zeros(F, np.int32))
    for f, r in enumerate(results):
        n = len(r["status"])
        for k in ("best_idx", "best_dist", "status", "other"):
            e[k][f, :n] = r[k]
        e["n_fused"][f] = r["n_fused"]
    a = dict(t, **p, tgt=np.array([i[0] for i in items], np.int32), list=np.array([i[1] for i in items], np.int32), cand=cand, n_cand=n_cand)
    sh = dict(n_tab=len(table), cap=cap, n_pts=n_pts, n_items=F, n_lists=len(cand), lcap=lcap)
    return a, sh, e


def debug_arrays(res, lcap):
    """What msl_debug_fuse returns for an item with the model's result res: the traces, zeros beyond the list."""
    out = {}
    for k, dt in (("u", F32), ("v", F32), ("ur", F32), ("level", np.int32), ("n_indices", np.int32)):
        out[k] = np.zeros(lcap, dt)
        out[k][:len(res["trace"])] = [tr[k] for tr in res["trace"]]
    return out


@functools.lru_cache(maxsize=None)
def p1():
    """P1.  Keyframe 1 of a table of three has 8192 keypoints; a quarter of its slots hold points, some of them bad.  The list has 65536
    entries over a point table of 1 << 20: about 4000 live candidates (most projected from a keypoint with a descriptor near its own, the
    rest anywhere, behind the camera, out of range, looking away), 600 ids the keyframe holds, 9000 bad ids, the rest NULL.  Placed by
    hand: three candidates on keypoint 8191 at j = 40000, 50000 and 65535; a candidate midway between the twin keypoints A and B, which
    share a descriptor and lie in neighbouring cells; three candidates in the hole of the keypoints; the ids 0 and 1048575; the smallest
    and the largest held id, and the two neighbours of a held id."""
    rng = np.random.default_rng(109)
    prm = fs.prm()
    cap, n_pts, lcap, tgt = MAX_CAP, MAX_PTS, MAX_LCAP, 1
    T = make_pose((0.05, -0.02, 0.03), (0.01, -0.02, 0.015))
    kf = _keyframe(rng, cap, T, HOLE)
    kp = kf["kps_un"]
    A, B, TOP = 100, 5000, cap - 1
    kp["x"][A], kp["y"][A] = 61.3, 70.2
    kp["x"][B], kp["y"][B] = 61.3 - 2.8, 70.2
    kp["octave"][[A, B]] = 1
    kf["uright"][[A, B]] = -1
    kf["desc"][B] = kf["desc"][A]
    pts = _point_table(n_pts)
    pts["flags"][:] = rng.random(n_pts) > 0.3
    pts["nobs"][:] = rng.integers(1, 11, n_pts)
    ids = rng.permutation(np.arange(2, n_pts - 2))
    held_pool, live, bad_ids = ids[:2048].copy(), ids[2048:2048 + 3990].copy(), ids[6100:300000]
    held_pool[0], held_pool[1] = 17, n_pts - 6                        # the smallest and the largest held id
    held_pool = held_pool[(held_pool == 17) | (held_pool == n_pts - 6) | ((held_pool > 17) & (held_pool < n_pts - 6))]
    hset = set(held_pool.tolist())
    mid = next(int(h) for h in held_pool[50:] if h - 1 not in hset and h + 1 not in hset)
    live = np.array([p for p in live if p not in hset and p not in (mid - 1, mid + 1)] + [0, n_pts - 1, mid - 1, mid + 1])
    slots = rng.permutation(np.setdiff1d(np.arange(cap), [A, B, TOP]))[:len(held_pool)]
    held = np.full(cap, -1, np.int32)
    held[slots] = held_pool
    pts["flags"][held_pool] = rng.random(len(held_pool)) > 0.15
    pts["flags"][live] = 1
    sf = prm["scale_factors"].astype(float)
    for n, p in enumerate(live):
        r = rng.random()
        if r < 0.75:                                                  # on a keypoint, nearly half of them on a slot that holds a point
            i = int(slots[rng.integers(0, len(slots))]) if rng.random() < 0.45 else int(rng.integers(0, cap))
            o = int(kp["octave"][i])
            noise = 0.4 * sf[o]
            u, v = float(kp["x"][i]) + rng.normal(0, noise), float(kp["y"][i]) + rng.normal(0, noise)
            bits = rng.integers(0, 13) if rng.random() < 0.8 else rng.integers(30, 70)
            _seen_point(rng, pts, p, T, min(max(u, 0.2), W - 0.2), min(max(v, 0.2), H - 0.2), o + int(rng.random() < 0.3 and o < 7),
                        _flip(kf["desc"][i], rng, bits), look_away=r < 0.03, short=0.03 <= r < 0.06)
        elif r < 0.9:                                                 # anywhere in the image, a descriptor of its own
            _seen_point(rng, pts, p, T, rng.uniform(1, W - 1), rng.uniform(1, H - 1), int(rng.integers(0, 8)), rng.integers(0, 256, 32, dtype=np.uint8))
        else:                                                         # anywhere around the camera: behind it, beside the image
            z = rng.uniform(-4, 6)
            pts["xyz"][p] = (rng.uniform(-1.5, 1.5) * z, rng.uniform(-1.2, 1.2) * z, z)
            pts["normal"][p] = (0, 0, 1); pts["dist"][p] = (0.5, 12.0); pts["desc"][p] = rng.integers(0, 256, 32, dtype=np.uint8)
    hits = [int(p) for p in live[10:13]]                              # three on keypoint 8191, its descriptor exactly
    for p in hits:
        _seen_point(rng, pts, p, T, float(kp["x"][TOP]), float(kp["y"][TOP]), int(kp["octave"][TOP]), kf["desc"][TOP].copy())
    twin = int(live[13])
    _seen_point(rng, pts, twin, T, 61.3 - 1.4, 70.2, 1, kf["desc"][A].copy())
    hole = [int(p) for p in live[14:17]]
    for p in hole:
        _seen_point(rng, pts, p, T, 115.0 + rng.uniform(-2, 2), 35.0 + rng.uniform(-2, 2), 0, rng.integers(0, 256, 32, dtype=np.uint8))
    pts["flags"][bad_ids[~np.isin(bad_ids, live)]] = 0
    pts["flags"][[17, n_pts - 6, mid]] = 1
    _finish_keyframe(kf, held)
    placed = hits + [twin] + hole + [0, n_pts - 1, mid - 1, mid + 1]
    retired = _retire(prm, kf, pts, [int(p) for p in live])
    # the list: every kind at random places, the three hits of keypoint 8191 at theirs
    lst = np.full(lcap, -1, np.int64)
    rest = np.array([p for p in live if p not in hits])
    entries = np.concatenate([rest, held_pool[:600], [17, n_pts - 6, mid], bad_ids[:9000]])
    entries = np.unique(entries)
    where = rng.permutation(np.setdiff1d(np.arange(lcap), [40000, 50000, lcap - 1]))[:len(entries)]
    lst[where] = entries[rng.permutation(len(entries))]
    lst[40000], lst[50000], lst[lcap - 1] = hits
    lst = [int(p) for p in lst]
    other = [_finish_keyframe(_keyframe(rng, 5, make_pose((0, 0, 0))), np.full(5, -1, np.int32)) for _ in range(2)]
    table = [other[0], kf, other[1]]
    res = fm.fuse_item(prm, kf, pts, lst)
    a, sh, e = _fuse_pack(table, pts, [(tgt, 0)], [lst], cap, lcap, [res])
    facts = dict(A=A, B=B, top=TOP, hits=hits, twin=twin, hole=hole, held_min=17, held_max=n_pts - 6, mid=mid, live=[int(p) for p in live],
                 retired=retired, placed=placed, ends=(0, n_pts - 1), n_live=len(live))
    return dict(a=a, sh=sh, e=e, facts=facts, res=[res], prm=prm, kf=kf, pts=pts, lst=lst, items=[(tgt, 0)])


@functools.lru_cache(maxsize=None)
def p2():
    """P2.  n_items = n_lists = n_tab = 4096, cap 16, lcap 12, 600 points.  Table keyframe k is distinct keyframe k % 37 and list l is distinct
    list l % 37; item f fuses list f into keyframe f, so the model runs on 37 items and item 4095 names keyframe 4095 and list 4095.
    Item 5 fuses list 4, which item 4 uses too: the model runs on that pair as well."""
    rng = np.random.default_rng(110)
    prm = fs.prm()
    cap, lcap, n_pts, n = 16, 12, 600, MAX_ITEMS
    pts = _point_table(n_pts)
    pts["flags"][:] = rng.random(n_pts) > 0.1
    pts["nobs"][:] = rng.integers(1, 11, n_pts)
    kfs, lists, retired, live = [], [], [], []
    free = iter(rng.permutation(n_pts).tolist())
    for r in range(PERIOD):
        T = make_pose(rng.uniform(-0.1, 0.1, 3), rng.uniform(-0.03, 0.03, 3))
        kf = _keyframe(rng, int(rng.integers(cap // 2, cap + 1)), T)
        nk = len(kf["kps_un"])
        held = np.full(nk, -1, np.int32)
        for i in range(nk):
            if rng.random() < 0.4:
                held[i] = next(free)
        _finish_keyframe(kf, held)
        lst = []
        for _ in range(int(rng.integers(lcap // 2, lcap + 1))):
            q = rng.random()
            if q < 0.1:
                lst.append(-1)
            elif q < 0.2 and (held >= 0).any():
                lst.append(int(rng.choice(held[held >= 0])))
            else:
                p = next(free)
                i = int(rng.integers(0, nk))
                o = int(kf["kps_un"]["octave"][i])
                _seen_point(rng, pts, p, T, float(kf["kps_un"]["x"][i]), float(kf["kps_un"]["y"][i]), o, _flip(kf["desc"][i], rng, rng.integers(0, 9)))
                lst.append(p)
        lst = list(dict.fromkeys(x for x in lst if x >= 0)) + [x for x in lst if x < 0]
        kfs.append(kf); lists.append(lst)
    pairs = [(r, r) for r in range(PERIOD)] + [(5, 4)]
    for t, l in pairs:
        cands = [p for p in lists[l] if p >= 0 and pts["flags"][p] & 1 and p not in set(kfs[t]["held_id"].tolist())]
        live += cands
        retired += _retire(prm, kfs[t], pts, cands)
    small = [fm.fuse_item(prm, kfs[t], pts, lists[l]) for t, l in pairs]
    table = [kfs[k % PERIOD] for k in range(n)]
    a, sh, e = _fuse_pack(kfs, pts, [(r, r) for r in range(PERIOD)], lists, cap, lcap, small[:PERIOD])
    for k in ("kps_un", "uright", "grid_cell", "desc", "n_kps", "Tcw", "held_id", "cand", "n_cand"):
        a[k] = tile(a[k], n)
    e = {k: tile(v, n) for k, v in e.items()}
    a["tgt"], a["list"] = np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32)
    a["list"][5] = 4
    _, _, e5 = _fuse_pack(kfs, pts, [(5, 4)], lists, cap, lcap, small[PERIOD:])
    for k in e:
        e[k][5] = e5[k][0]
    sh = dict(sh, n_tab=n, n_items=n, n_lists=n)
    facts = dict(period=PERIOD, shared=(4, 5), retired=retired, n_live=len(set(live)), pairs=pairs)
    return dict(a=a, sh=sh, e=e, facts=facts, res=small, prm=prm, kfs=kfs, pts=pts, lists=lists, table=table)


# ---- msl_fuse_map_lines ----------------------------------------------------------------------------------------------------------------
def _line_keyframe(rng, n, T):
    """n random keylines on the 320 x 240 image of tests/linefuse_scenes.py."""
    from manhattanslam_amd import KEYLINE_DTYPE
    kl = np.zeros(n, KEYLINE_DTYPE)
    kl["x"], kl["y"] = rng.uniform(30, ls.W - 30, n), rng.uniform(30, ls.H - 30, n)
    kl["angle"], kl["octave"] = rng.uniform(-1.5, 1.5, n), rng.integers(0, 8, n)
    return dict(kl=kl, ldesc=rng.integers(0, 256, (n, 32), dtype=np.uint8), Tcw=T, held_id=np.full(n, -1, np.int32))


def _line_world(T, u, v, z):
    R, t = T[:, :3].astype(float), T[:, 3].astype(float)
    return R.T @ (np.array([(u - ls.CX) / ls.FX * z, (v - ls.CY) / ls.FY * z, z]) - t)


def _seen_line(rng, lines, p, kf, i, level, desc, look_away=False, short=False, off=(0.0, 0.0)):
    """Line p of the table: its projection has its midpoint at keyline i of kf (moved by off) and a slope below the keyline's angle, its
    distance range predicts `level`, its normal looks at the camera."""
    T, kl = kf["Tcw"], kf["kl"][i]
    s = float(kl["angle"]) - rng.uniform(0.05, 0.6)
    du = rng.uniform(8, 25) / np.sqrt(1 + s * s)
    x, y = float(kl["x"]) + off[0], float(kl["y"]) + off[1]
    P = np.concatenate([_line_world(T, x - du, y - s * du, rng.uniform(3, 5)), _line_world(T, x + du, y + s * du, rng.uniform(3, 5))])
    P = np.round(P * 4096.0) / 4096.0                                 # exact in float, and so is the midpoint
    view = 0.5 * (P[:3] + P[3:]) + T[:, :3].astype(float).T @ T[:, 3].astype(float)
    d = np.linalg.norm(view)
    dmax = d * 1.2 ** (level - rng.uniform(0.2, 0.8)) * (0.3 if short else 1.0)
    lines["xyz"][p], lines["normal"][p] = P, (-1 if look_away else 1) * view / d
    lines["dist"][p], lines["desc"][p] = (dmax / 1.2 ** 7, dmax), desc


def _line_table(n):
    return dict(xyz=np.zeros((n, 6), np.float64), normal=np.zeros((n, 3), np.float64), dist=np.zeros((n, 2), F32), desc=np.zeros((n, 32), np.uint8),
                flags=np.zeros(n, np.uint8), nobs=np.zeros(n, np.int32))


def _retire_lines(prm, kf, lines, live):
    gone = []
    for p in live:
        m = []
        lf.search_one(prm, kf, lines["xyz"][p], lines["normal"][p], lines["dist"][p], lines["desc"][p], m, {})
        if any(abs(lhs - rhs) <= MARGIN * abs(scale) for _, lhs, rhs, scale in m):
            lines["flags"][p] = 0
            gone.append(int(p))
    return gone


def line_margins(prm, kf, lines, lst):
    m = []
    lf.fuse_item(prm, kf, lines, lst, margins=m)
    return m


def _lfuse_pack(table, lines, items, lists, klcap, lcap, results):
    from manhattanslam_amd import fuse, linefuse
    _, t = linefuse.pack_line_table(table, klcap)
    n_lines, p = linefuse.pack_lines(lines)
    _, cand, n_cand = fuse.pack_lists(lists, lcap)
    F = len(items)
    e = dict(best_idx=np.full((F, lcap), -1, np.int32), best_dist=np.zeros((F, lcap), np.int32), status=np.zeros((F, lcap), np.uint8),
             other=np.full((F, lcap), -1, np.int32), n_fused=np.zeros(F, np.int32))
    for f, r in enumerate(results):
        n = len(r["status"])
        for k in ("best_idx", "best_dist", "status", "other"):
            e[k][f, :n] = r[k]
        e["n_fused"][f] = r["n_fused"]
    a = dict(t, **{k: p[k] for k in linefuse.LINE_KEYS}, tgt=np.array([i[0] for i in items], np.int32), list=np.array([i[1] for i in items], np.int32),
             cand=cand, n_cand=n_cand)
    return a, dict(n_tab=len(table), klcap=klcap, n_lines=n_lines, n_items=F, n_lists=len(cand), lcap=lcap), e


def line_debug_arrays(res, lcap):
    """What msl_debug_line_fuse returns for an item with the model's result res."""
    out = {}
    for k, dt in (("u1", F32), ("v1", F32), ("u2", F32), ("v2", F32), ("radius", F32), ("level", np.int32), ("n_indices", np.int32)):
        out[k] = np.zeros(lcap, dt)
        out[k][:len(res["trace"])] = [tr[k] for tr in res["trace"]]
    return out


@functools.lru_cache(maxsize=None)
def l1():
    """L1.  Keyframe 1 of three has 256 keylines, half of them holding lines (some bad).  The list has 65536 entries over a line table of
    1 << 20: about 2500 live candidates (three in four projected onto a keyline with a descriptor near its own, the rest anywhere), 9000
    bad ids, the rest NULL; lines the keyframe holds are candidates like any other.  Placed by hand: three candidates on keyline 255 at
    j = 40000, 50000 and 65535; on keyline 40 the line it holds, then two more (SELF, a replacement, UNRESOLVED); on the empty keyline 41
    a line the keyframe holds at keyline 200; the ids 0 and 1048575."""
    rng = np.random.default_rng(111)
    prm = ls.prm()
    klcap, n_lines, lcap, tgt = MAX_KLCAP, MAX_PTS, MAX_LCAP, 1
    T = make_pose((0.05, -0.02, 0.03), (0.01, -0.02, 0.015))
    kf = _line_keyframe(rng, klcap, T)
    lines = _line_table(n_lines)
    lines["flags"][:] = rng.random(n_lines) > 0.3
    lines["nobs"][:] = rng.integers(1, 11, n_lines)
    ids = rng.permutation(np.arange(1, n_lines - 1))
    TOP, SELF_KL, EMPTY_KL, ELSEWHERE = klcap - 1, 40, 41, 200
    held_pool, live, bad_ids = ids[:128].copy(), ids[128:128 + 2490], ids[3000:300000]
    slots = rng.permutation(np.setdiff1d(np.arange(klcap), [TOP, SELF_KL, EMPTY_KL, ELSEWHERE]))[:126]
    slots = np.concatenate([slots, [SELF_KL, ELSEWHERE]])
    kf["held_id"][slots] = held_pool
    lines["flags"][held_pool] = rng.random(128) > 0.15
    own, twice = int(kf["held_id"][SELF_KL]), int(kf["held_id"][ELSEWHERE])
    lines["flags"][[own, twice]] = 1
    live = np.concatenate([live, [0, n_lines - 1], held_pool[:60]])   # sixty held lines are candidates too, `own` and `twice` among them
    live = np.unique(np.concatenate([live, [own, twice]]))
    lines["flags"][live[~np.isin(live, held_pool)]] = 1
    anyone = np.setdiff1d(np.arange(klcap), [TOP, SELF_KL, EMPTY_KL])     # the keylines of the placed candidates are theirs alone
    for p in live:
        r = rng.random()
        if r < 0.75:
            i = int(slots[rng.integers(0, 126)]) if rng.random() < 0.5 else int(anyone[rng.integers(0, len(anyone))])
            o = int(kf["kl"]["octave"][i])
            bits = rng.integers(0, 13) if rng.random() < 0.8 else rng.integers(30, 70)
            level = o + (1 if rng.random() < 0.3 and o < 7 else 0) + (3 if rng.random() < 0.05 else 0)
            _seen_line(rng, lines, p, kf, i, level, _flip(kf["ldesc"][i], rng, bits), look_away=r < 0.03, short=0.03 <= r < 0.06,
                       off=rng.normal(0, 0.4 * 1.2 ** o, 2))
        elif r < 0.9:
            i = int(anyone[rng.integers(0, len(anyone))])
            _seen_line(rng, lines, p, kf, i, int(rng.integers(0, 8)), rng.integers(0, 256, 32, dtype=np.uint8), off=rng.uniform(-25, 25, 2))
        else:
            z = rng.uniform(-4, 6, 2)
            lines["xyz"][p] = np.round(np.concatenate([rng.uniform(-1.2, 1.2, 2) * z[0], z[:1], rng.uniform(-1.2, 1.2, 2) * z[1], z[1:]]) * 4096) / 4096
            lines["normal"][p] = (0, 0, 1); lines["dist"][p] = (0.5, 12.0); lines["desc"][p] = rng.integers(0, 256, 32, dtype=np.uint8)
    fresh = [int(p) for p in live if p not in set(held_pool.tolist()) and p not in (0, n_lines - 1)]
    hits, after_self = fresh[10:13], fresh[13:15]
    exact = lambda p, i: _seen_line(rng, lines, p, kf, i, int(kf["kl"]["octave"][i]), kf["ldesc"][i].copy())
    for p in hits:
        exact(p, TOP)
    for p in [own] + after_self:
        exact(p, SELF_KL)
    exact(twice, EMPTY_KL)
    exact(0, 7); exact(n_lines - 1, 9)
    lines["flags"][bad_ids[~np.isin(bad_ids, live)]] = 0
    placed = hits + [own] + after_self + [twice, 0, n_lines - 1]
    retired = _retire_lines(prm, kf, lines, [int(p) for p in live if lines["flags"][p] & 1])
    n_live = int((lines["flags"][live] & 1).sum()) + len(retired)
    special = hits + [own] + after_self
    entries = np.unique(np.concatenate([[p for p in live if p not in special], bad_ids[:9000]]))
    lst = np.full(lcap, -1, np.int64)
    fixed = [40000, 50000, lcap - 1, 1000, 2000, 3000]
    where = rng.permutation(np.setdiff1d(np.arange(lcap), fixed))[:len(entries)]
    lst[where] = entries[rng.permutation(len(entries))]
    lst[fixed] = special
    lst = [int(p) for p in lst]
    other = [_line_keyframe(rng, 5, make_pose((0, 0, 0))) for _ in range(2)]
    table = [other[0], kf, other[1]]
    res = lf.fuse_item(prm, kf, lines, lst)
    a, sh, e = _lfuse_pack(table, lines, [(tgt, 0)], [lst], klcap, lcap, [res])
    facts = dict(top=TOP, self_kl=SELF_KL, empty_kl=EMPTY_KL, elsewhere=ELSEWHERE, hits=hits, own=own, after_self=after_self, twice=twice,
                 retired=retired, placed=placed, n_live=n_live, ends=(0, n_lines - 1))
    return dict(a=a, sh=sh, e=e, facts=facts, res=[res], prm=prm, kf=kf, lines=lines, lst=lst)


@functools.lru_cache(maxsize=None)
def l2():
    """L2.  n_items = n_lists = n_tab = 4096, klcap 12, lcap 10, 600 lines, tiled as P2: keyframe k is distinct keyframe k % 37, list l is
    distinct list l % 37, item f fuses list f into keyframe f; item 5 fuses list 4, which item 4 uses too."""
    rng = np.random.default_rng(112)
    prm = ls.prm()
    klcap, lcap, n_lines, n = 12, 10, 600, MAX_ITEMS
    lines = _line_table(n_lines)
    lines["flags"][:] = rng.random(n_lines) > 0.1
    lines["nobs"][:] = rng.integers(1, 11, n_lines)
    kfs, lists, retired, live = [], [], [], []
    free = iter(rng.permutation(n_lines).tolist())
    for r in range(PERIOD):
        kf = _line_keyframe(rng, int(rng.integers(klcap // 2, klcap + 1)), make_pose(rng.uniform(-0.1, 0.1, 3), rng.uniform(-0.03, 0.03, 3)))
        nk = len(kf["kl"])
        for i in range(nk):
            if rng.random() < 0.4:
                kf["held_id"][i] = next(free)
        lst = []
        for _ in range(int(rng.integers(lcap // 2, lcap + 1))):
            q = rng.random()
            i = int(rng.integers(0, nk))
            if q < 0.1:
                lst.append(-1)
                continue
            p = int(kf["held_id"][i]) if q < 0.25 and kf["held_id"][i] >= 0 else next(free)
            _seen_line(rng, lines, p, kf, i, int(kf["kl"]["octave"][i]), _flip(kf["ldesc"][i], rng, rng.integers(0, 9)))
            lst.append(p)
        lst = list(dict.fromkeys(x for x in lst if x >= 0)) + [x for x in lst if x < 0]
        kfs.append(kf); lists.append(lst)
    pairs = [(r, r) for r in range(PERIOD)] + [(5, 4)]
    for t, l in pairs:
        cands = [p for p in lists[l] if p >= 0 and lines["flags"][p] & 1]
        live += cands
        retired += _retire_lines(prm, kfs[t], lines, cands)
    small = [lf.fuse_item(prm, kfs[t], lines, lists[l]) for t, l in pairs]
    a, sh, e = _lfuse_pack(kfs, lines, [(r, r) for r in range(PERIOD)], lists, klcap, lcap, small[:PERIOD])
    for k in ("kl", "ldesc", "n_kl", "Tcw", "held_id", "cand", "n_cand"):
        a[k] = tile(a[k], n)
    e = {k: tile(v, n) for k, v in e.items()}
    a["tgt"], a["list"] = np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32)
    a["list"][5] = 4
    _, _, e5 = _lfuse_pack(kfs, lines, [(5, 4)], lists, klcap, lcap, small[PERIOD:])
    for k in e:
        e[k][5] = e5[k][0]
    sh = dict(sh, n_tab=n, n_items=n, n_lists=n)
    facts = dict(period=PERIOD, shared=(4, 5), retired=retired, n_live=len(set(live)), pairs=pairs)
    return dict(a=a, sh=sh, e=e, facts=facts, res=small, prm=prm, kfs=kfs, lines=lines, lists=lists)


# ---- msl_refresh_map_lines -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def r3():
    """R3.  n_lines 1 << 20, klcap 256, n_tab 4096: 3000 lines with 1 .. 12 observations, the ids 0 and 1048575 among them, a few bad lines
    and a few without observations.  Keyframe 4095 and keyline 255 are observed, and are reference keyframe and reference keyline of the
    last id, whose range ends at n_obs_total."""
    from manhattanslam_amd import linefuse
    rng = np.random.default_rng(113)
    n_tab, klcap, n_lines = MAX_TAB, MAX_KLCAP, MAX_PTS
    prm = mm.params()
    table = [_line_keyframe(rng, klcap, make_pose(rng.uniform(-1, 1, 3) * (0.8, 0.3, 0.5), rng.uniform(-0.1, 0.1, 3))) for _ in range(n_tab)]
    real = np.unique(np.concatenate([[0, n_lines - 1], rng.integers(1, n_lines - 1, 3000)]))
    obs = {int(p): [(int(k), int(rng.integers(0, klcap))) for k in rng.permutation(n_tab)[:int(rng.integers(1, 13))]] for p in real}
    obs[n_lines - 1] = [(0, 5), (n_tab - 1, klcap - 1), (1, klcap - 1)]
    obs[0] = [(n_tab - 1, 0), (2, klcap - 1)]
    flags = np.zeros(n_lines, np.uint8)
    flags[real] = 1
    dead = np.unique(rng.integers(1, n_lines - 1, 40))
    dead = dead[~np.isin(dead, real)]
    empty = real[5:45:4]
    for p in empty:
        obs[int(p)] = []
    xyz = np.zeros((n_lines, 6), np.float64)
    z = rng.uniform(2, 6, (len(real), 2))
    xyz[real] = np.concatenate([rng.uniform(-0.6, 0.6, (len(real), 2)) * z[:, :1], z[:, :1], rng.uniform(-0.6, 0.6, (len(real), 2)) * z[:, 1:], z[:, 1:]], 1)
    ref = np.zeros(n_lines, np.int32)
    for p in real:
        o = obs[int(p)]
        ref[p] = o[int(rng.integers(0, len(o)))][0] if o and rng.random() < 0.8 else int(rng.integers(0, n_tab))
    ref[n_lines - 1] = n_tab - 1
    ids = np.concatenate([real, dead]).astype(np.int32)
    ids = ids[rng.permutation(len(ids))]
    F = len(ids)
    e = dict(out_normal=np.zeros((F, 3), np.float64), out_dist=np.zeros((F, 2), F32), status=np.zeros(F, np.uint8),
             ln_normal=filled((n_lines, 3), np.float64), ln_dist=filled((n_lines, 2), F32))
    for f, p in enumerate(ids):
        p = int(p)
        e["status"][f], e["out_normal"][f], e["out_dist"][f] = lf.update_average_dir(prm, table, xyz[p], obs.get(p, []), int(ref[p]), not flags[p])
        if e["status"][f] == lf.NORMAL_WRITTEN:
            e["ln_normal"][p], e["ln_dist"][p] = e["out_normal"][f], e["out_dist"][f]
    _, t = linefuse.pack_line_table(table, klcap)
    a = dict({k: t[k] for k in linefuse.REFRESH_TABLE_KEYS}, **_csr({p: o for p, o in obs.items() if o}, n_lines), ln_xyz=xyz, ln_flags=flags,
             ln_ref=ref, ids=ids)
    sh = dict(n_tab=n_tab, klcap=klcap, n_lines=n_lines, n_items=F, n_obs_total=int(a["obs_off"][-1]))
    return dict(a=a, sh=sh, e=e, facts=dict(obs=obs, dead=dead, empty=empty, prm=prm, last_kf=n_tab - 1, last_idx=klcap - 1))


# ---- msl_triangulate_new_points --------------------------------------------------------------------------------------------------------
def _tri_pack(table, items, cap, ncap, results):
    """Packed inputs of msl_triangulate_new_points and the expected arrays from one create_new_map_points result per item."""
    from manhattanslam_amd import triangulate
    _, t = triangulate.pack_table(table, cap)
    _, cur, neigh, n_neigh = triangulate.pack_items(items, ncap)
    F = len(items)
    e = triangulate.outputs(F, ncap, cap)
    for k in ("match12", "new_neigh", "new_idx2", "new_order"):
        e[k][:] = -1
    for f, r in enumerate(results):
        R, n1, nn = len(r["nmatches"]), len(r["new_neigh"]), len(r["new_order"])
        e["match12"][f, :R, :n1], e["status"][f, :R, :n1], e["nmatches"][f, :R] = r["match12"], r["status"], r["nmatches"]
        for k in ("new_neigh", "new_idx2", "new_xyz", "new_normal", "new_dist", "new_desc"):
            e[k][f, :n1] = r[k]
        e["new_order"][f, :nn], e["n_new"][f] = r["new_order"], nn
    a = dict(t, cur=cur, neigh=neigh, n_neigh=n_neigh)
    return a, dict(n_tab=len(table), cap=cap, n_items=F, ncap=ncap), e


def _empty_keyframe():
    return dict(kps_un=np.zeros(0, KP), raw_xy=np.zeros((0, 2), F32), uright=np.zeros(0, F32), depth=np.zeros(0, F32), desc=np.zeros((0, 32), np.uint8),
                node=np.zeros(0, np.int32), held=np.zeros(0, np.uint8), Tcw=make_pose((0, 0, 0)))


T1_SEED, T2_SEED = 120, 130


@functools.lru_cache(maxsize=None)
def t1():
    """T1.  Seventeen keyframes on an arc inside a table of 4096 whose other keyframes have no keypoints; the orientation check is on.  The
    current keyframe is table index 4095 and its sixteen neighbours, in order, sit at 0, 4094 and fourteen indices in between; the
    neighbour of rank 8 stands 2 cm from the current keyframe and is skipped for its baseline.  Every point is seen by the current
    keyframe and by a random third of the others, the first eight by rank 0 and rank 12 both, and eight more by rank 15 alone."""
    r = np.random.RandomState(T1_SEED)
    n_kf, skipped = 17, 8
    poses = [make_pose((0.15 * k, 0.03 * np.sin(k), 0.02 * np.cos(2 * k)), (0.0, -0.01 * k, 0.0)) for k in range(n_kf)]
    poses[1 + skipped] = make_pose((0.02, 0.01, 0.0))
    B = ts.Builder(T1_SEED + 1, poses)
    pts = ts._points(r, 86, 2.0, 5.0, 0.35) + np.array([1.2, 0, 0])
    for i, X in enumerate(pts):
        views = [0] + [k for k in range(1, n_kf) if r.uniform() < 0.3]
        if i < 8:
            views = sorted(set(views) | {1, 13})
        elif i < 16:
            views = [0, 16]
        if len(views) >= 2:
            B.track(X, views, held=[k for k in views if r.uniform() < 0.1 and i >= 16], tag="p%d" % i)
    for k in range(n_kf):
        B.clutter(k, 4)
    small = B.finish()
    where = [MAX_TAB - 1, 0, MAX_TAB - 2] + [int(k) for k in np.sort(r.choice(np.arange(1, MAX_TAB - 2), n_kf - 3, replace=False))]
    nothing = _empty_keyframe()
    table = [nothing] * MAX_TAB
    for k, w in enumerate(where):
        table[w] = small[k]
    items = [(where[0], where[1:])]
    prm = ts.prm(check_orientation=True)
    margins = []
    res = [tm.create_new_map_points(prm, table, c, nb, margins=margins) for c, nb in items]
    cap = max(len(k["kps_un"]) for k in small)
    a, sh, e = _tri_pack(table, items, cap, 16, res)
    return dict(a=a, sh=sh, e=e, facts=dict(where=where, skipped=skipped, retired=[], n_live=sum(len(k["kps_un"]) for k in small)), res=res, prm=prm,
                items=items, margins=margins, table=table)


@functools.lru_cache(maxsize=None)
def t2():
    """T2.  n_items 65535, cap 8, ncap 2, a table of 111 keyframes: 37 distinct items, each a keyframe of its own with two neighbours of its
    own (the second is sometimes skipped for its baseline), tiled with period 37."""
    r = np.random.RandomState(T2_SEED)
    n, cap = 65535, 8
    table, items = [], []
    for q in range(PERIOD):
        near = q % 5 == 3
        poses = [make_pose((0, 0, 0)), make_pose((0.35 + r.uniform(-0.05, 0.05), r.uniform(-0.05, 0.05), 0.02), (0.0, -0.03, 0.0)),
                 make_pose((0.02, 0.01, 0.0)) if near else make_pose((-0.3, r.uniform(-0.05, 0.05), 0.0), (0.0, 0.04, 0.0))]
        B = ts.Builder(T2_SEED + 1 + q, poses)
        for X in ts._points(r, int(r.randint(3, 7)), 2.5, 4.0, 0.3):
            B.track(X, [0] + [k for k in (1, 2) if r.uniform() < 0.8], node=int(r.randint(0, 3)))
        for k in range(3):
            B.clutter(k, cap - len(B.feats[k]) if q % 7 == 0 else 1, node_range=(0, 3))
        items.append((len(table), [len(table) + 1, len(table) + 2][:1 if q % 6 == 5 else 2]))
        table += B.finish()
    prm = ts.prm()
    margins = []
    res = [tm.create_new_map_points(prm, table, c, nb, margins=margins) for c, nb in items]
    a, sh, e = _tri_pack(table, items, cap, 2, res)
    for k in ("cur", "neigh", "n_neigh"):
        a[k] = tile(a[k], n)
    e = {k: tile(v, n) for k, v in e.items()}
    return dict(a=a, sh=dict(sh, n_items=n), e=e, facts=dict(period=PERIOD, retired=[], n_live=sum(len(k["kps_un"]) for k in table)), res=res, prm=prm,
                items=items, margins=margins, table=table)

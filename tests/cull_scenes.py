"""Scenes for the culling entries: random keyframe graphs and hand-built ones, one per pin (tests/cull_model.py describes the scene dict),
their packing into the ABI's arrays, the arrays the model expects of a call, and the call in its three forms."""
import numpy as np

from tests import cull_model as cm
from tests.localmap_scenes import FILL, DevArray, device_filled, host_filled, same  # noqa: F401

K, C, O, N = cm.KEPT, cm.CULLED, cm.ORIGIN, cm.NOT_ERASE


# ---- building ----------------------------------------------------------------------------------------------------------------------------
def graph(n_tab, th_depth=40.0, origin=None):
    """A scene of n_tab keyframes without slots or points."""
    e = lambda: [[] for _ in range(n_tab)]
    return dict(held=e(), octave=e(), uright=e(), depth=e(), kf_bad=[False] * n_tab, not_erase=[False] * n_tab, pt_bad=[], pt_nobs=[],
                pt_obs=[], origin=origin, th_depth=th_depth, items=[])


def add_slot(s, k, p, octave=0, stereo=True, depth=1.0):
    """A new slot of keyframe k holding point p (None = NULL); returns its index."""
    s["held"][k].append(p); s["octave"][k].append(octave); s["uright"][k].append(10.0 if stereo else -1.0); s["depth"][k].append(depth)
    return len(s["held"][k]) - 1


def add_point(s, observers, bad=False, nobs=None):
    """A point observed by `observers`, each a keyframe k or (k, octave, stereo) and each holding it in a new slot (octave 0, stereo, depth
    1 unless given); Observations() is the sum of the weights unless nobs is given.  Returns its id."""
    p = len(s["pt_bad"])
    s["pt_bad"].append(bad); s["pt_obs"].append([]); s["pt_nobs"].append(0)
    for o in observers:
        k, octave, stereo = (o, 0, True) if isinstance(o, int) else o
        s["pt_obs"][p].append((k, add_slot(s, k, p, octave, stereo)))
        s["pt_nobs"][p] += 2 if stereo else 1
    if nobs is not None:
        s["pt_nobs"][p] = nobs
    return p


def fill(s, k, n, others):
    """n points held and observed by k and by the keyframes in `others` (three or more make them redundant for k)."""
    return [add_point(s, [k] + list(others)) for _ in range(n)]


# ---- the pins: each returns the scene and, per item, the rows the sequential function must give ------------------------------------------
def pin_cull_ends_redundancy():
    """1. Culling A makes B, redundant on entry, no longer redundant."""
    s = graph(4)
    fill(s, 0, 10, [1, 2, 3])
    s["items"] = [[0, 1]]
    return s, [[(10, 10, 0, C), (10, 0, 0, K)]]


def pin_cull_turns_points_bad():
    """2. Culling A turns B's two weak points bad; the ten left are all redundant: B is culled with n_gone 2."""
    s = graph(5)
    fill(s, 0, 20, [2, 3, 4]); fill(s, 1, 10, [2, 3, 4])
    for _ in range(2):
        add_point(s, [0, (1, 0, False)])                                  # nObs 3: one stereo erasure leaves 1
    s["items"] = [[0, 1], [1]]
    return s, [[(22, 20, 0, C), (10, 10, 2, C)], [(12, 10, 0, K)]]


def pin_mono_and_stereo_erasure():
    """3. Q is observed by A1 (mono), A2 (stereo) and B (mono), nObs 4.  Culling A1 leaves 3: Q stays, B has 9 of 10 and is kept.  Culling A2
    leaves 2: Q turns bad, B has 9 of 9 and is culled."""
    s = graph(6)
    fill(s, 0, 20, [3, 4, 5]); fill(s, 1, 20, [3, 4, 5]); fill(s, 2, 9, [3, 4, 5])
    add_point(s, [(0, 0, False), (1, 0, True), (2, 0, False)])
    s["items"] = [[0, 2], [1, 2]]
    return s, [[(21, 20, 0, C), (10, 9, 0, K)], [(21, 20, 0, C), (9, 9, 1, C)]]


def pin_nobs_boundary():
    """4. Observations() exactly 4 and exactly 3 at B's turn: Observations() of both points is 5 on entry, A's erasure takes 1 (mono) and 2
    (stereo); each keeps three qualifying observers."""
    s = graph(5)
    fill(s, 0, 20, [2, 3, 4])
    m = lambda k: (k, 0, False)
    add_point(s, [m(0), m(1), m(2), m(3), m(4)])
    add_point(s, [0, m(1), m(2), m(3), m(4)], nobs=5)
    s["items"] = [[0, 1]]
    return s, [[(22, 22, 0, C), (2, 1, 0, K)]]


def pin_octave_boundary():
    """5. B's slots are at octave 2.  Once A is gone the first point keeps three observers at octave 3 = octave + 1 and is redundant, the
    second keeps two at 3 and one at 4 = octave + 2 and is not."""
    s = graph(5)
    fill(s, 0, 20, [2, 3, 4])
    add_point(s, [0, (1, 2, True), (2, 3, True), (3, 3, True), (4, 3, True)])
    add_point(s, [0, (1, 2, True), (2, 3, True), (3, 3, True), (4, 4, True)])
    s["items"] = [[0, 1]]
    return s, [[(22, 20, 0, C), (2, 1, 0, K)]]                            # at A's octave 0 neither point has a qualifying observer


def pin_nine_tenths():
    """6. 9 of 10 is kept, 10 of 11 is culled: one point of each loses its third observer with A."""
    s = graph(6)
    fill(s, 0, 20, [3, 4, 5]); fill(s, 1, 9, [3, 4, 5]); fill(s, 2, 10, [3, 4, 5])
    add_point(s, [0, 1, 3, 4]); add_point(s, [0, 2, 3, 4])
    s["items"] = [[0, 1, 2]]
    return s, [[(22, 22, 0, C), (10, 9, 0, K), (11, 10, 0, C)]]


def pin_no_points_left():
    """7. n_mps == 0 keeps the keyframe: both of B's points turn bad with A; C has no slots at all."""
    s = graph(6)
    fill(s, 0, 30, [3, 4, 5])
    for _ in range(2):
        add_point(s, [0, (1, 0, False)])
    s["items"] = [[0, 1, 2]]
    return s, [[(32, 30, 0, C), (0, 0, 2, K), (0, 0, 0, K)]]


def pin_origin():
    """8. The origin is skipped without counting, although every point it holds is redundant; its observations stay, so B is culled.
    The second item puts A in front: C loses its third observer with A."""
    s = graph(7, origin=1)
    fill(s, 1, 10, [2, 4, 5])                                             # origin and B share these; X, Y observe them
    fill(s, 0, 20, [4, 5, 6])
    for _ in range(3):
        add_point(s, [0, 3, 4, 5])
    s["items"] = [[1, 2], [0, 1, 2, 3]]
    return s, [[(0, 0, 0, O), (10, 10, 0, C)], [(23, 23, 0, C), (0, 0, 0, O), (10, 10, 0, C), (3, 0, 0, K)]]


def pin_not_erase():
    """9. N is redundant but mbNotErase: its observations stay, so B, which needs them, is culled as on entry; C loses its third observer
    with A."""
    s = graph(7)
    s["not_erase"][1] = True
    fill(s, 1, 10, [2, 4, 5])
    fill(s, 0, 20, [4, 5, 6])
    for _ in range(3):
        add_point(s, [0, 3, 4, 5])
    s["items"] = [[0, 1, 2, 3]]
    return s, [[(23, 23, 0, C), (10, 10, 0, N), (10, 10, 0, C), (3, 0, 0, K)]]


def pin_point_in_two_slots():
    """10. A and B each hold R in two slots.  A's erasure happens once (nObs 5 - 2 = 3, R stays); B counts R twice, not redundant."""
    s = graph(5)
    fill(s, 0, 30, [2, 3, 4]); fill(s, 1, 8, [2, 3, 4])
    m = lambda k: (k, 0, False)
    r = add_point(s, [0, m(1), m(2), m(3)])
    add_slot(s, 0, r); add_slot(s, 1, r, stereo=False)
    s["items"] = [[0, 1]]
    return s, [[(32, 32, 0, C), (10, 8, 0, K)]]


def pin_inconsistent_tables():
    """11. A holds U, which does not observe A: untouched.  V observes A at an empty slot, A does not hold it: the observation stays and
    still counts for B.  W is consistent and loses A."""
    s = graph(6)
    fill(s, 0, 20, [3, 4, 5])
    m = lambda k: (k, 0, False)
    u = add_point(s, [m(1), m(3), m(4), m(5)])
    add_slot(s, 0, u, stereo=False)
    v = add_point(s, [m(1), m(3), m(4)])
    s["pt_obs"][v].append((0, add_slot(s, 0, None, stereo=False))); s["pt_nobs"][v] += 1
    add_point(s, [0, 1, 3, 4])
    s["items"] = [[0, 1]]
    return s, [[(22, 22, 0, C), (3, 2, 0, K)]]


def pin_long_observation_list():
    """12. More than 64 observations: 66 at octave 5 first, the qualifying ones at the end of the list, A among them."""
    s = graph(72)
    far = [(k, 5, True) for k in range(6, 72)]
    fill(s, 0, 20, [2, 3, 4])
    add_point(s, far + [0, 1, 2, 3])
    add_point(s, far + [0, 1, 2, 3, 4])
    s["items"] = [[0, 1]]
    return s, [[(22, 22, 0, C), (2, 1, 0, K)]]


def pin_empty_and_full_rows():
    """13. n_cand of 0 and of ccap (4)."""
    s = graph(7)
    fill(s, 0, 10, [1, 2, 3]); fill(s, 4, 5, [1, 5, 6])
    s["items"] = [[], [0, 1, 4, 2]]
    return s, [[], [(10, 10, 0, C), (15, 5, 0, K), (5, 5, 0, C), (10, 0, 0, K)]]


def pin_nan_depth():
    """14. The literal depth tests: NaN, th and 0 count; th + 1 and -1 do not."""
    s = graph(4, th_depth=3.5)
    pts = fill(s, 0, 5, [1, 2, 3])
    s["depth"][0][:5] = [float("nan"), 4.5, -1.0, 3.5, 0.0]
    assert [s["held"][0][i] for i in range(5)] == pts
    s["items"] = [[0]]
    return s, [[(3, 3, 0, C)]]


def pin_observation_at_another_slot():
    """15. Q observes A at an empty mono slot while A holds Q in another, stereo slot: A holds it, so the observation is erased, by the
    weight of the observation's keypoint (4 - 1 = 3: Q stays and is not redundant; the slot's weight would turn it bad)."""
    s = graph(5)
    fill(s, 0, 20, [2, 3, 4])
    m = lambda k: (k, 0, False)
    q = add_point(s, [m(1), m(2), m(3)])
    s["pt_obs"][q].append((0, add_slot(s, 0, None, stereo=False))); s["pt_nobs"][q] += 1
    add_slot(s, 0, q, stereo=True)
    s["items"] = [[0, 1]]
    return s, [[(21, 21, 0, C), (1, 0, 0, K)]]


PINS = [pin_cull_ends_redundancy, pin_cull_turns_points_bad, pin_mono_and_stereo_erasure, pin_nobs_boundary, pin_octave_boundary, pin_nine_tenths,
        pin_no_points_left, pin_origin, pin_not_erase, pin_point_in_two_slots, pin_inconsistent_tables, pin_long_observation_list,
        pin_empty_and_full_rows, pin_nan_depth, pin_observation_at_another_slot]


# ---- random graphs -----------------------------------------------------------------------------------------------------------------------
def random_scene(seed, n_tab, cap, n_items=2, ccap=None, inconsistent=0.05):
    """A keyframe graph whose keyframes fall into a few anchors, which also hold the weakly observed points, and the rest, whose points are
    mostly observed five times and more: the rest is culled one after the other until the survivors' points run short of observers.
    Stereo and mono keypoints are mixed; `inconsistent`: the share of slots that hold a point without its observation, and of
    observations at an empty slot of a keyframe that does not hold the point."""
    rng = np.random.default_rng(seed)
    s = graph(n_tab, th_depth=8.0, origin=int(rng.integers(0, n_tab)) if rng.random() < 0.7 else None)
    ccap = ccap or n_tab
    s["kf_bad"] = [bool(rng.random() < 0.1) for _ in range(n_tab)]
    s["not_erase"] = [bool(rng.random() < 0.1) for _ in range(n_tab)]
    n_slots = [int(rng.integers(cap // 2, cap + 1)) for _ in range(n_tab)]
    anchors, n_weak = max(1, n_tab // 4), [0] * n_tab

    def slot(k, p):
        d = rng.random()
        depth = float("nan") if d < 0.01 else -1.0 if d < 0.04 else 9.0 if d < 0.08 else float(rng.uniform(0, 8))
        return add_slot(s, k, p, int(rng.choice([0, 1, 1, 1, 2])), bool(rng.random() < 0.6), depth)

    for _ in range(max(1, int(sum(n_slots) * 0.85 / 5))):
        weak = rng.random() < 0.2
        n_obs = int(rng.integers(1, 4)) if weak else int(rng.integers(5, 10))
        pool = rng.permutation(n_tab)
        if weak and anchors >= 2:                                         # among the anchors, and every other time in one keyframe of the rest
            pool = list(rng.permutation(anchors)[:n_obs - 1])
            rest = [k for k in range(anchors, n_tab) if n_weak[k] < max(1, n_slots[k] // 14)]
            if rest and rng.random() < 0.8:
                pool.append(rest[int(rng.integers(0, len(rest)))]); n_weak[pool[-1]] += 1
        p = len(s["pt_bad"])
        s["pt_bad"].append(bool(rng.random() < 0.05)); s["pt_obs"].append([]); s["pt_nobs"].append(0)
        for k in pool[:n_obs]:
            k = int(k)
            if len(s["held"][k]) >= n_slots[k]:
                continue
            r = rng.random()
            if r < inconsistent:                                          # an observation at an empty slot: k does not hold the point
                idx = slot(k, None)
            else:
                idx = slot(k, p)
                if r < 2 * inconsistent:                                  # held without the observation
                    continue
            s["pt_obs"][p].append((k, idx))
            s["pt_nobs"][p] += 2 if s["uright"][k][idx] >= 0 else 1
    n_pts = len(s["pt_bad"])
    for k in range(n_tab):                                                # a second slot for a point of the keyframe, and NULL slots
        while len(s["held"][k]) < n_slots[k]:
            mine = [p for p in s["held"][k] if p is not None]
            slot(k, int(rng.choice(mine)) if mine and rng.random() < 0.1 else None if rng.random() < 0.9 else int(rng.integers(0, n_pts)))
    for _ in range(n_items):
        n = int(rng.integers(max(1, ccap // 2), ccap + 1))
        s["items"].append([int(k) for k in rng.permutation(n_tab)[:n]])
    return s


# ---- packing, the expected arrays, the call ----------------------------------------------------------------------------------------------
def pack(scene, cap=None, ccap=None):
    """The scene as the arrays of msl.h (a dict keyed by the argument names) and its shape (a dict)."""
    from manhattanslam_amd import KEYPOINT_DTYPE, mappoint
    n_tab, n_pts, items = len(scene["held"]), max(len(scene["pt_bad"]), 1), scene["items"]
    cap = cap or max([len(h) for h in scene["held"]] + [1])
    ccap = ccap or max([len(c) for c in items] + [1])
    a = dict(kps_un=np.zeros((n_tab, cap), KEYPOINT_DTYPE), uright=np.full((n_tab, cap), -1, np.float32), depth=np.full((n_tab, cap), -1, np.float32),
             held_id=np.full((n_tab, cap), -1, np.int32), n_kps=np.array([len(h) for h in scene["held"]], np.int32),
             kf_flags=np.array([(0 if b else 1) | (2 if ne else 0) for b, ne in zip(scene["kf_bad"], scene["not_erase"])], np.uint8),
             pt_flags=np.array([0 if b else 1 for b in scene["pt_bad"]] + [0] * (n_pts - len(scene["pt_bad"])), np.uint8),
             pt_nobs=np.array(list(scene["pt_nobs"]) + [0] * (n_pts - len(scene["pt_nobs"])), np.int32),
             cand=np.full((len(items), ccap), -1, np.int32), n_cand=np.array([len(c) for c in items], np.int32))
    for k in range(n_tab):
        n = len(scene["held"][k])
        a["kps_un"]["octave"][k, :n] = scene["octave"][k]
        a["uright"][k, :n], a["depth"][k, :n] = scene["uright"][k], scene["depth"][k]
        a["held_id"][k, :n] = [-1 if p is None else p for p in scene["held"][k]]
    for f, c in enumerate(items):
        a["cand"][f, :len(c)] = c
    o = mappoint.pack_observations(list(scene["pt_obs"]) or [[]])
    a.update(obs_off=o["obs_off"], obs_kf=o["obs_kf"], obs_idx=o["obs_idx"])
    return a, dict(n_tab=n_tab, cap=cap, n_pts=n_pts, n_items=len(items), n_obs_total=int(o["obs_off"][-1]), ccap=ccap,
                   origin=-1 if scene["origin"] is None else scene["origin"], th_depth=scene["th_depth"])


def model(scene):
    """cull_keyframes of every item: [(rows, order)]."""
    return [cm.cull_keyframes(scene, c) for c in scene["items"]]


def expected(sh, want):
    """The arrays a call leaves in outputs that held FILL, from the model's rows."""
    F, ccap = sh["n_items"], sh["ccap"]
    e = dict(n_mps=np.full((F, ccap), -1, np.int32), n_redundant=np.full((F, ccap), -1, np.int32), n_gone=np.full((F, ccap), -1, np.int32),
             status=np.zeros((F, ccap), np.uint8))
    for f, (rows, _) in enumerate(want):
        for r, row in enumerate(rows[:ccap]):
            e["n_mps"][f, r], e["n_redundant"][f, r], e["n_gone"][f, r], e["status"][f, r] = row
    return e


def run(a, sh, mem=0, handle=None, keep=None):
    """msl_cull_keyframes: mem = 0 on host arrays, 1 on DevArrays (a handle is needed).  The outputs hold FILL before.  Returns every
    output as a numpy array; keep (a dict) receives the arrays as they were passed."""
    from manhattanslam_amd import cull
    d = {k: DevArray(v) for k, v in a.items()} if mem else dict(a)
    out = cull.keyframes_outputs(sh["n_items"], sh["ccap"], device_filled if mem else host_filled)
    cull.cull_keyframes(cull.cull_params(sh["th_depth"]), sh["n_tab"], sh["cap"], sh["n_pts"], sh["n_items"], sh["n_obs_total"], sh["ccap"],
                        sh["origin"], d, out, mem, handle=handle)
    if handle is not None:
        handle.sync()
    if keep is not None:
        keep.update(d); keep.update(out)
    return {k: (v.numpy() if mem else v) for k, v in out.items()}

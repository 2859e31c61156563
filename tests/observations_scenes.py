"""Scenes for msl_observations_apply: random maps and logs, one hand-built scene per pin of msl.h, the too-long scenes, their packing into
the ABI's arrays, the arrays the model expects of a call, and the call in its forms.  A scene is (state, ops) as tests/observations_model.py
describes them."""
import numpy as np

from tests import observations_model as om
from tests.localmap_scenes import FILL, DevArray, device_filled, host_filled, same  # noqa: F401

A, E, B, R, K = om.ADD, om.ERASE, om.SET_BAD, om.REPLACE, om.KF_ERASE


# ---- building ----------------------------------------------------------------------------------------------------------------------------
def empty(n_tab, cap, n_pts, stereo=None, lines=False):
    """A map of n_tab keyframes with cap slots each (all inside n_kps) and n_pts points without observations: live, nObs 0, reference -1.
    stereo: the slots with uright >= 0 as a boolean [n_tab][cap] (default: the even ones); lines: no uright at all."""
    if stereo is None:
        stereo = np.arange(n_tab * cap).reshape(n_tab, cap) % 2 == 0
    return dict(n_kps=np.full(n_tab, cap, np.int32), uright=None if lines else np.where(stereo, 10.0, -1.0).astype(np.float32),
                held_id=np.full((n_tab, cap), -1, np.int32), pt_flags=np.full(n_pts, 5, np.uint8), pt_nobs=np.zeros(n_pts, np.int32),
                pt_ref=np.full(n_pts, -1, np.int32), pt_found=np.zeros(n_pts, np.int32), pt_visible=np.zeros(n_pts, np.int32),
                pt_replaced=np.full(n_pts, -1, np.int32), obs=[[] for _ in range(n_pts)])


def observe(s, p, k, i, hold=True):
    """Point p observes keyframe k at keypoint i (and k holds it there): nObs by the weight; the first observer is the reference."""
    s["obs"][p] = sorted(s["obs"][p] + [(k, i)])
    s["pt_nobs"][p] += 1 if s["uright"] is None else 2 if s["uright"][k][i] >= 0 else 1
    if s["pt_ref"][p] < 0:
        s["pt_ref"][p] = k
    if hold:
        s["held_id"][k][i] = p


def kill(s, p):
    """A point that is bad on entry: no observations."""
    assert not s["obs"][p]
    s["pt_flags"][p] &= 0xFE


# ---- the pins: each returns (state, ops) ---------------------------------------------------------------------------------------------------
def pin_add_new_and_known():
    """ADD of a new observation goes to its sorted place and writes the slot; ADD of a keyframe the point observes leaves the list and
    nObs alone and still writes the slot it names."""
    s = empty(4, 4, 3)
    observe(s, 0, 1, 0); observe(s, 0, 3, 1)
    return s, [(A, 0, 2, 3), (A, 0, 0, 2), (A, 0, 3, 2), (A, 2, 1, 1)]


def pin_add_on_a_bad_point():
    """No bad test: a bad point takes the observation and the slot, and stays bad."""
    s = empty(3, 3, 2)
    kill(s, 1)
    return s, [(A, 1, 2, 0), (A, 1, 0, 1)]


def pin_erase_reference_and_last():
    """ERASE of the reference keyframe moves the reference to the first keyframe left; of the last observation, to -1; of a keyframe the
    point does not observe, nothing.  The points keep nObs above 2 (a wide nObs on entry), so none turns bad."""
    s = empty(4, 4, 3)
    for k in (1, 2, 3):
        observe(s, 0, k, 0)
    s["pt_ref"][0] = 2
    observe(s, 1, 2, 1)
    s["pt_nobs"][:2] = [9, 9]
    return s, [(E, 0, 2), (E, 0, 0), (E, 1, 2), (E, 2, 1)]


def pin_erase_cascade():
    """nObs 4 (two stereo): one erasure leaves 2, the point turns bad, its other slot is NULLed, nObs stays 2; a later ERASE and ADD on it."""
    s = empty(3, 4, 2)
    observe(s, 0, 0, 0); observe(s, 0, 2, 2)
    observe(s, 1, 0, 1); observe(s, 1, 1, 0); observe(s, 1, 2, 0)         # mono, stereo, stereo: 5 - 2 = 3 stays
    return s, [(E, 0, 2), (E, 1, 1), (E, 0, 0), (A, 0, 1, 2)]


def pin_set_bad():
    """SET_BAD clears bit 0 alone, NULLs every observed slot, empties the range and keeps nObs; a second one changes nothing."""
    s = empty(3, 3, 2)
    observe(s, 0, 0, 1); observe(s, 0, 1, 2); observe(s, 1, 2, 0)
    return s, [(B, 0), (B, 0), (B, 1)]


def pin_replace():
    """REPLACE: the survivor takes the keyframes it does not observe, the shared keyframe's slot of the replaced point is NULLed, found and
    visible are added, a == b does nothing."""
    s = empty(4, 4, 3)
    observe(s, 0, 0, 0); observe(s, 0, 1, 1); observe(s, 0, 3, 3)
    observe(s, 1, 1, 2); observe(s, 1, 2, 0)
    s["pt_found"][:2], s["pt_visible"][:2] = [3, 10], [7, 20]
    return s, [(R, 1, 1), (R, 0, 1), (R, 2, 2)]


def pin_replace_chain():
    """REPLACE(0, 1) then REPLACE(1, 2) then REPLACE(3, 2): the second moves what the first brought; the third meets keyframe 0 in the
    survivor only because of the chain (the survivor's observations on entry do not have it)."""
    s = empty(4, 4, 4)
    observe(s, 0, 0, 0); observe(s, 0, 1, 0)
    observe(s, 1, 2, 0)
    observe(s, 2, 3, 0)
    observe(s, 3, 0, 1); observe(s, 3, 3, 1)
    return s, [(R, 0, 1), (R, 1, 2), (R, 3, 2)]


def pin_slot_written_twice():
    """Several ops write one slot: the last in log order wins, whatever it writes."""
    s = empty(3, 3, 4)
    observe(s, 0, 1, 1)
    return s, [(A, 1, 1, 1), (A, 2, 1, 1), (B, 0), (A, 3, 2, 0), (A, 1, 2, 0), (B, 3)]


def pin_kf_erase():
    """KF_ERASE walks the slots: a point held twice is erased once, a stale slot (the point does not observe the keyframe) and a NULL slot
    do nothing, a weak point turns bad and frees its slot in the next keyframe, whose own KF_ERASE then finds an empty range."""
    s = empty(4, 6, 5)
    for k in (0, 1, 2, 3):
        observe(s, 0, k, 0)                                               # strong
    observe(s, 1, 0, 1); observe(s, 1, 1, 1)                              # weak: mono + mono
    s["held_id"][0][2] = 0                                                # held twice
    s["held_id"][0][3] = 2                                                # stale: point 2 observes keyframe 3 only
    observe(s, 2, 3, 1); observe(s, 2, 2, 2); observe(s, 2, 1, 2)
    observe(s, 3, 1, 3); observe(s, 3, 2, 3); observe(s, 3, 3, 3)
    return s, [(K, 0, 0), (K, 0, 1), (A, 4, 3, 4), (E, 3, 2)]


def pin_lines():
    """The MapLine form: uright NULL, every weight 1; pt_found / pt_visible / pt_replaced left out."""
    s = empty(3, 3, 3, lines=True)
    for k in (0, 1, 2):
        observe(s, 0, k, 0)
    observe(s, 1, 1, 1)
    s["pt_found"] = s["pt_visible"] = s["pt_replaced"] = None
    return s, [(K, 0, 2), (A, 2, 0, 2), (R, 1, 0), (E, 0, 0)]


def pin_kf_erase_inconsistent_pair():
    """The one case in which the slots on entry are not the live walk (msl.h's pin): point 0 turns bad in KF_ERASE(0) and NULLs the slot of
    its observation in keyframe 1 -- a slot that holds point 1, which observes keyframe 1 at another, empty slot.  KeyFrame::SetBadFlag on
    keyframe 1 then no longer meets point 1; the entry walks the slots on entry, erases its observation and turns it bad."""
    s = empty(3, 4, 2)
    observe(s, 0, 0, 0); observe(s, 0, 1, 1, hold=False)                  # stereo + mono: the erasure leaves 1
    s["held_id"][1][1] = 1
    observe(s, 1, 1, 2, hold=False); observe(s, 1, 2, 0)                  # stereo + stereo: an erasure leaves 2
    return s, [(K, 0, 0), (K, 0, 1)]


PINS = [pin_add_new_and_known, pin_add_on_a_bad_point, pin_erase_reference_and_last, pin_erase_cascade, pin_set_bad, pin_replace,
        pin_replace_chain, pin_slot_written_twice, pin_kf_erase, pin_lines]


ALL_SEEDS, LINE_SEEDS = range(24), range(100, 104)


def all_scenes():
    """Every scene on which the slots on entry are the live walk, as (name, function): the pins, the random maps, the line maps.  The model
    tests and the GPU tests run the same list; pin_kf_erase_inconsistent_pair is run beside it."""
    return [(pin.__name__, pin) for pin in PINS] + [(f"random{seed}", lambda seed=seed: random_scene(seed)) for seed in ALL_SEEDS] + \
           [(f"lines{seed}", lambda seed=seed: random_scene(seed, lines=True)) for seed in LINE_SEEDS]


# ---- too long ------------------------------------------------------------------------------------------------------------------------------
def long_map(with_300=True):
    """n_tab 260, cap 2: point 0 with 256 observations, point 1 with 300, point 2 with 255, point 3 with two keyframes point 2 lacks and
    one it has, point 4 new.  300 observations in 260 keyframes repeat keyframes: a range no host-memory call accepts and no op may name,
    which a device-memory call copies (with_300 = False leaves the point empty)."""
    s = empty(260, 2, 5)
    for k in range(256):
        observe(s, 0, k, 0)
    if with_300:
        s["obs"][1] = [(j % 260, 1) for j in range(300)]
        s["pt_nobs"][1], s["pt_ref"][1] = 300, 0
    for k in range(255):
        observe(s, 2, k, 1, hold=False)
    observe(s, 3, 100, 0, hold=False); observe(s, 3, 257, 0); observe(s, 3, 258, 0)
    return s


LONG = dict(erase_at_the_limit=[(E, 0, 17), (A, 0, 259, 0)], add_beyond=[(A, 4, 3, 0), (A, 0, 259, 0), (E, 0, 3)], replace_beyond=[(R, 3, 2)],
            replace_at_the_limit=[(E, 3, 258), (R, 3, 2)], named_long=[(A, 4, 3, 0), (E, 1, 5), (B, 1)])
LONG_COUNTS = dict(erase_at_the_limit=0, add_beyond=1, replace_beyond=1, replace_at_the_limit=0, named_long=1)


# ---- random maps and logs ------------------------------------------------------------------------------------------------------------------
def random_scene(seed, n_tab=None, cap=None, n_pts=None, n_ops=None, lines=False):
    """A seeded map -- points observed by one to n_tab keyframes with stereo and mono keypoints mixed, bad points, new rows, points held in
    two slots of a keyframe, stale slots -- and a log: KF_ERASEs in front, then ADDs (new, repeated, on bad points), ERASEs (observed or
    not, of the reference, of the last observation), SET_BADs and REPLACEs, with chains through a survivor."""
    rng = np.random.default_rng(seed)
    n_tab = n_tab or int(rng.integers(4, 7)); cap = cap or int(rng.integers(5, 9))
    n_pts = n_pts or int(rng.integers(12, 41)); n_ops = n_ops or int(rng.integers(20, 65))
    s = empty(n_tab, cap, n_pts, stereo=rng.random((n_tab, cap)) < 0.5, lines=lines)
    s["n_kps"] = rng.integers(max(1, cap - 2), cap + 1, n_tab).astype(np.int32)
    s["pt_flags"] = rng.choice([1, 5, 7], n_pts).astype(np.uint8)
    s["pt_found"], s["pt_visible"] = rng.integers(0, 9, n_pts).astype(np.int32), rng.integers(0, 30, n_pts).astype(np.int32)
    free = [[i for i in range(s["n_kps"][k])] for k in range(n_tab)]
    for p in range(n_pts):
        r = rng.random()
        if r < 0.15:                                                      # a new row, or a bad point
            if r < 0.08:
                kill(s, p)
            continue
        for k in rng.permutation(n_tab)[:int(rng.integers(1, n_tab + 1))]:
            if free[k]:
                observe(s, p, int(k), free[k].pop(int(rng.integers(0, len(free[k])))), hold=rng.random() < 0.9)
        if s["obs"][p] and rng.random() < 0.5:
            s["pt_ref"][p] = s["obs"][p][int(rng.integers(0, len(s["obs"][p])))][0]
        if rng.random() < 0.2:
            s["pt_nobs"][p] += int(rng.integers(1, 4))                    # a counter the table does not explain
    for k in range(n_tab):                                                # a second slot for a held point, and stale slots
        for i in free[k]:
            r = rng.random()
            mine = [int(p) for p in s["held_id"][k] if p >= 0]
            if r < 0.3 and mine:
                s["held_id"][k][i] = mine[int(rng.integers(0, len(mine)))]
            elif r < 0.5:
                s["held_id"][k][i] = int(rng.integers(0, n_pts))
    pt = lambda: int(rng.integers(0, n_pts))
    kf = lambda: int(rng.integers(0, n_tab))
    ops = [(K, 0, kf()) for _ in range(int(rng.integers(0, 3)))]
    hub = pt()
    while len(ops) < n_ops:
        r, p, k = rng.random(), pt(), kf()
        if r < 0.35:
            ops.append((A, p, k, int(rng.integers(0, s["n_kps"][k]))))
            if rng.random() < 0.2:
                ops.append(ops[-1])
        elif r < 0.6:
            o = s["obs"][p]
            ops.append((E, p, o[int(rng.integers(0, len(o)))][0] if o and rng.random() < 0.8 else k))
        elif r < 0.7:
            ops.append((B, p))
        else:
            q = hub if rng.random() < 0.4 else pt()
            ops.append((R, p, q))
            if rng.random() < 0.3:
                hub = pt()
                ops.append((R, q, hub))
    return s, ops[:n_ops]


# ---- scenes from the other models ----------------------------------------------------------------------------------------------------------
def from_cull_scene(scene):
    """A tests/cull_model.py scene as a state: observation lists ascending by keyframe, a point that is bad on entry without observations
    (as cull_model.build_objects reads it), the reference keyframe the first observer."""
    n_tab, n_pts = len(scene["held"]), max(len(scene["pt_bad"]), 1)
    cap = max([len(h) for h in scene["held"]] + [1])
    s = empty(n_tab, cap, n_pts)
    s["n_kps"] = np.array([len(h) for h in scene["held"]], np.int32)
    for k in range(n_tab):
        n = len(scene["held"][k])
        s["uright"][k, :n] = scene["uright"][k]
        s["held_id"][k, :n] = [-1 if p is None else p for p in scene["held"][k]]
    for p, bad in enumerate(scene["pt_bad"]):
        s["pt_flags"][p], s["pt_nobs"][p] = 0 if bad else 1, scene["pt_nobs"][p]
        s["obs"][p] = [] if bad else sorted(scene["pt_obs"][p])
        s["pt_ref"][p] = s["obs"][p][0][0] if s["obs"][p] else -1
    return s


def from_fuse_graph(g):
    """A tests/fuse_model.py Graph as a state (no found / visible counters there)."""
    n_tab, n_pts = len(g.kfs), len(g.mps)
    cap = max(len(kf.slots) for kf in g.kfs)
    s = empty(n_tab, cap, n_pts)
    s["n_kps"] = np.array([len(kf.slots) for kf in g.kfs], np.int32)
    s["pt_found"] = s["pt_visible"] = None
    for kf in g.kfs:
        s["uright"][kf.id, :len(kf.slots)] = kf.data["uright"]
        s["held_id"][kf.id, :len(kf.slots)] = [-1 if m is None else m.id for m in kf.slots]
    for mp in g.mps:
        s["obs"][mp.id] = sorted(mp.obs.items())
        s["pt_flags"][mp.id], s["pt_nobs"][mp.id] = 0 if mp.bad else 1, mp.nobs
        s["pt_ref"][mp.id] = s["obs"][mp.id][0][0] if mp.obs else -1
        s["pt_replaced"][mp.id] = -1 if mp.replaced is None else mp.replaced.id
    return s


class _Slots(list):
    """KeyFrame.slots that tells the recorder of every assignment."""

    def __init__(self, items, kid, rec):
        super().__init__(items)
        self.kid, self.rec = kid, rec

    def __setitem__(self, idx, mp):
        self.rec.slot(self.kid, idx, mp)
        super().__setitem__(idx, mp)


class _Recorder:
    """The statements fuse_model.replay makes on the objects, as a log: a top-level add_observation with the slot assignment behind it is an
    ADD, a top-level replace a REPLACE; what they do inside (the survivor's add_observation, the slots they write) is the op's own."""

    def __init__(self):
        self.ops, self.depth, self.pending = [], 0, None

    def slot(self, kid, idx, mp):
        if self.depth == 0:
            assert self.pending == (mp.id, kid, idx), "a slot assignment that is not the AddMapPoint of the AddObservation before it"
            self.ops.append((A,) + self.pending)
            self.pending = None


def record_fuse_log(name):
    """fuse_model.replay on the graph `name` of tests/fuse_scenes.py with the objects' methods wrapped: (the state on entry, the log, the
    graph afterwards)."""
    from tests import fuse_model as fm
    from tests import fuse_scenes as fs
    g, prm, cur, targets = fs.graph(name)
    entry, rec = from_fuse_graph(g), _Recorder()
    for kf in g.kfs:
        kf.slots = _Slots(kf.slots, kf.id, rec)
    add, replace = fm.MapPoint.add_observation, fm.MapPoint.replace

    def add_observation(self, kf, idx):
        if rec.depth == 0:
            assert rec.pending is None
            rec.pending = (self.id, kf.id, int(idx))
        return add(self, kf, idx)

    def replace_(self, other):
        assert rec.depth == 0 and rec.pending is None
        rec.ops.append((R, self.id, other.id))
        rec.depth += 1
        try:
            return replace(self, other)
        finally:
            rec.depth -= 1

    fm.MapPoint.add_observation, fm.MapPoint.replace = add_observation, replace_
    try:
        fm.replay(g, prm, cur, targets)
    finally:
        fm.MapPoint.add_observation, fm.MapPoint.replace = add, replace
    assert rec.pending is None
    return entry, rec.ops, g


# ---- packing, the expected arrays, the call ------------------------------------------------------------------------------------------------
def pack(state, ops, ocap=None, tcap=None):
    """The scene as the arrays of msl.h (a dict keyed by the argument names) and its shape (a dict)."""
    from manhattanslam_amd import observations
    off, okf, oidx = om.csr(state["obs"])
    n_tab, cap = state["held_id"].shape
    n_add = sum(1 for o in ops if o[0] == A)
    a = {k: None if state[k] is None else np.ascontiguousarray(state[k]) for k in ("n_kps", "uright", "held_id") + om.POINT_KEYS}
    a.update(obs_off=off, obs_kf=okf if len(okf) else np.zeros(1, np.int32), obs_idx=oidx if len(oidx) else np.zeros(1, np.int32),
             ops=observations.pack_ops(ops))
    n_pts = len(state["pt_flags"])
    return a, dict(n_tab=n_tab, cap=cap, n_pts=n_pts, n_obs_total=int(off[-1]), n_ops=len(ops), ocap=int(off[-1]) + n_add if ocap is None else ocap,
                   tcap=n_pts if tcap is None else tcap)


def expected(a, sh, want):
    """The arrays a call leaves -- in-place arrays from `a`, outputs that held FILL -- from the model's result `want`.  With a too-long
    point op_status and touched are unspecified and left out."""
    from manhattanslam_amd import observations
    e = {k: np.array(want["state"][k]) for k in observations.INOUT_KEYS if a[k] is not None}
    out = observations.outputs(sh["n_pts"], sh["n_ops"], sh["ocap"], sh["tcap"], host_filled)
    out["counts"][:] = want["counts"]
    if want["counts"][2]:
        del out["op_status"], out["touched"]
    else:
        off, okf, oidx = om.csr(want["state"]["obs"])
        out["obs_off_out"][:] = off
        out["obs_kf_out"][:len(okf)], out["obs_idx_out"][:len(oidx)] = okf, oidx
        out["op_status"][:] = want["op_status"]
        out["touched"][:] = (want["touched"] + [-1] * sh["tcap"])[:sh["tcap"]]
    e.update(out)
    return e


def run(a, sh, mem=0, handle=None, keep=None):
    """msl_observations_apply: mem = 0 on copies of the host arrays, 1 on DevArrays (a handle is needed).  The outputs hold FILL before.
    Returns every in-place array and output as a numpy array; keep (a dict) receives the arrays as they were passed."""
    from manhattanslam_amd import observations
    d = {k: None if v is None else DevArray(v) if mem else v.copy() for k, v in a.items()}
    out = observations.outputs(sh["n_pts"], sh["n_ops"], sh["ocap"], sh["tcap"], device_filled if mem else host_filled)
    observations.apply(sh["n_tab"], sh["cap"], sh["n_pts"], sh["n_obs_total"], sh["n_ops"], sh["ocap"], sh["tcap"], d, d, out, mem, handle=handle)
    if handle is not None:
        handle.sync()
    if keep is not None:
        keep.update({k: v for k, v in d.items() if v is not None}); keep.update(out)
    got = {k: d[k] for k in observations.INOUT_KEYS if d[k] is not None}
    got.update(out)
    return {k: (v.numpy() if mem else v) for k, v in got.items()}

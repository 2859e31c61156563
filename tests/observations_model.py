"""Sequential models of msl_observations_apply (include/msl.h): a log of observation edits executed in order.

A state is a dict over one map:
  n_kps[k], uright[k][i] (or None: every weight 1, the MapLine form), held_id[k][i]     numpy arrays, the keyframe table (-1 = NULL)
  pt_flags, pt_nobs, pt_ref, pt_found, pt_visible, pt_replaced                          numpy arrays per point (the last three may be None)
  obs[p]                                                                                mObservations as a list of (keyframe, keypoint),
                                                                                        ascending by keyframe: std::map's order with pointer
                                                                                        order pinned to table order
An op is a tuple (op, a, b, c) as msl_obs_op; shorter tuples are padded with 0.

apply is the array model msl_observations_apply is compared with, byte for byte.  apply_literal is its twin on objects -- MapPoint with an
observation map, KeyFrame with its slots -- written from src/MapPoint.cc:83-187, src/KeyFrame.cc:185-197 and :362-368 of the reference;
tests/test_observations_model.py proves them equal, and proves the log against tests/cull_model.py and tests/fuse_model.py."""
import copy

import numpy as np

ADD, ERASE, SET_BAD, REPLACE, KF_ERASE = 1, 2, 3, 4, 5
CHANGED, TURNED_BAD = 1, 2
OBS_MAX, MAX_OPS, MAX_KF_ERASE = 256, 65536, 256
POINT_KEYS = ("pt_flags", "pt_nobs", "pt_ref", "pt_found", "pt_visible", "pt_replaced")
WRONG = ("slot_order", "no_cascade", "entry_survivor", "add_skips_slot", "append")


def pad(op):
    return tuple(int(x) for x in op) + (0,) * (4 - len(op))


def copy_state(s):
    return {k: (copy.deepcopy(v) if k == "obs" else None if v is None else np.array(v)) for k, v in s.items()}


def csr(obs):
    """obs_off, obs_kf, obs_idx of a list of observation lists."""
    off = np.zeros(len(obs) + 1, np.int32)
    off[1:] = np.cumsum([len(o) for o in obs])
    flat = [x for o in obs for x in o]
    return off, np.array([k for k, _ in flat], np.int32), np.array([i for _, i in flat], np.int32)


def point_view(s, p):
    """Everything of point p that `touched` and MSL_OBS_CHANGED compare."""
    return (tuple(s["obs"][p]),) + tuple(None if s[k] is None else int(s[k][p]) for k in POINT_KEYS)


# ---- the array model ---------------------------------------------------------------------------------------------------------------------
def apply(state, ops, wrong=None, slots="entry"):
    """The log executed in order on a copy of `state`.  Returns dict(state=, op_status=, touched=, counts=): the state on exit, one status
    per op, the ascending ids that differ from entry (all of them: the caller cuts at tcap) and counts[4].  If a point is too long the
    state is the entry's, counts is [n_obs_total, 0, n_long, 0] and op_status and touched are None.
    slots: what a KF_ERASE walks -- "entry", the slots the keyframe held on entry, which is msl.h's contract and what the device does, or
    "live", the slots as the ops before it left them, which is KeyFrame::SetBadFlag and the literal twin.  The two differ only on the
    inconsistent pair msl.h pins (tests/observations_scenes.py::pin_kf_erase_inconsistent_pair).
    wrong: one of WRONG, an implementation the scenes must tell from the right one."""
    assert slots in ("entry", "live")
    assert wrong is None or wrong in WRONG
    s, entry = copy_state(state), state
    n_tab, n_pts, cap = len(s["n_kps"]), len(s["pt_flags"]), s["held_id"].shape[1]
    obs, held = s["obs"], s["held_id"]
    named, too_long, slot_log, status, n_bad = set(), set(), [], [], [0]
    i32 = lambda x: int(np.int32(np.uint32(x & 0xFFFFFFFF)))

    def weight(k, i):
        return 1 if s["uright"] is None else 2 if s["uright"][k][i] >= 0 else 1

    def write(k, i, v):
        slot_log.append((k, i, v))
        if wrong != "slot_order":
            held[k][i] = v

    def name(p):                                                          # an op names p: False if the point is, or was, too long
        if p not in named:
            named.add(p)
            if len(obs[p]) > OBS_MAX:
                too_long.add(p)
        return p not in too_long

    def insert(p, k, i):
        obs[p].append((k, i))
        if wrong != "append":
            obs[p].sort()
        s["pt_nobs"][p] += weight(k, i)

    def set_bad(p):
        n_bad[0] += int(s["pt_flags"][p] & 1)
        s["pt_flags"][p] &= 0xFE
        for k, i in obs[p]:
            write(k, i, -1)
        obs[p] = []

    def erase(p, k, cascade=True):
        if not name(p):
            return
        at = [j for j, (kk, _) in enumerate(obs[p]) if kk == k]
        if not at:
            return
        s["pt_nobs"][p] -= weight(*obs[p][at[0]])
        del obs[p][at[0]]
        if s["pt_ref"][p] == k:
            s["pt_ref"][p] = min(kk for kk, _ in obs[p]) if obs[p] else -1
        if s["pt_nobs"][p] <= 2 and cascade:
            set_bad(p)

    n_kf_erase = 0
    for op, a, b, c in (pad(o) for o in ops):
        a_ok, kf_ok = 0 <= a < n_pts, 0 <= b < n_tab
        watch = [a] if a_ok else []
        if op == REPLACE and 0 <= b < n_pts:
            watch.append(b)
        if op == KF_ERASE and kf_ok:
            row = (entry["held_id"] if slots == "entry" else held)[b]
            watch = sorted({int(p) for p in row[:max(0, min(int(s["n_kps"][b]), cap))] if 0 <= p < n_pts})
        before = [point_view(s, p) for p in watch]
        if op == ADD and a_ok and kf_ok and 0 <= c < max(0, min(int(s["n_kps"][b]), cap)):
            if name(a):
                seen = any(k == b for k, _ in obs[a])
                if not seen and len(obs[a]) == OBS_MAX:
                    too_long.add(a)
                else:
                    if not seen:
                        insert(a, b, c)
                    if not (seen and wrong == "add_skips_slot"):
                        write(b, c, a)
        elif op == ERASE and a_ok and kf_ok:
            erase(a, b)
        elif op == SET_BAD and a_ok:
            if name(a):
                set_bad(a)
        elif op == REPLACE and a_ok and 0 <= b < n_pts and a != b:
            ok_a, ok_b = name(a), name(b)
            if ok_a and ok_b:
                theirs = {k for k, _ in (entry["obs"][b] if wrong == "entry_survivor" else obs[b])}
                moved = [(k, i) for k, i in obs[a] if k not in theirs]
                if len(obs[b]) + len(moved) > OBS_MAX:
                    too_long.add(b)
                else:
                    n_bad[0] += int(s["pt_flags"][a] & 1)
                    s["pt_flags"][a] &= 0xFE
                    if s["pt_replaced"] is not None:
                        s["pt_replaced"][a] = b
                    taken, obs[a] = obs[a], []
                    for k, i in taken:
                        if k not in theirs:
                            write(k, i, b)
                            insert(b, k, i)
                        else:
                            write(k, i, -1)
                    if s["pt_found"] is not None:
                        s["pt_found"][b] = i32(int(s["pt_found"][b]) + int(s["pt_found"][a]))
                        s["pt_visible"][b] = i32(int(s["pt_visible"][b]) + int(s["pt_visible"][a]))
        elif op == KF_ERASE and kf_ok and n_kf_erase < MAX_KF_ERASE:
            n_kf_erase += 1
            for i in range(max(0, min(int(s["n_kps"][b]), cap))):         # KeyFrame::SetBadFlag walks the live slots
                p = int((entry["held_id"] if slots == "entry" else held)[b][i])
                if 0 <= p < n_pts:
                    erase(p, b, cascade=wrong != "no_cascade")
        after = [point_view(s, p) for p in watch]
        st = CHANGED if before != after else 0
        if any(x[1] & 1 and not y[1] & 1 for x, y in zip(before, after)):
            st |= TURNED_BAD
        status.append(st)
    if wrong == "slot_order":
        for k, i, v in reversed(slot_log):
            held[k][i] = v
    n_total = sum(len(o) for o in entry["obs"])
    if too_long:
        return dict(state=copy_state(entry), op_status=None, touched=None, counts=[n_total, 0, len(too_long), 0])
    touched = [p for p in range(n_pts) if point_view(s, p) != point_view(entry, p)]
    return dict(state=s, op_status=status, touched=touched, counts=[sum(len(o) for o in obs), len(touched), 0, n_bad[0]])


# ---- the literal twin --------------------------------------------------------------------------------------------------------------------
class MapPoint:
    def __init__(self, pid, flags, nobs, found, visible):
        self.id, self.bad, self.other_bits, self.nobs, self.found, self.visible = pid, not flags & 1, flags & 0xFE, nobs, found, visible
        self.obs, self.ref, self.replaced = {}, None, None                # mObservations: KeyFrame -> idx; mpRefKF; mpReplaced

    def ordered(self, obs=None):                                          # std::map iterates in key order: pointer order = table order
        obs = self.obs if obs is None else obs
        return sorted(obs.items(), key=lambda kv: kv[0].k)

    def add_observation(self, kf, idx):                                   # src/MapPoint.cc:83-93
        if kf in self.obs:
            return
        self.obs[kf] = idx
        self.nobs += 2 if kf.uright[idx] >= 0 else 1

    def erase_observation(self, kf):                                      # :95-119
        bad = False
        if kf in self.obs:
            idx = self.obs[kf]
            self.nobs -= 2 if kf.uright[idx] >= 0 else 1
            del self.obs[kf]
            if self.ref is kf:
                self.ref = self.ordered()[0][0] if self.obs else None     # pin: mObservations.begin() of an empty map
            if self.nobs <= 2:
                bad = True
        if bad:
            self.set_bad_flag()

    def set_bad_flag(self):                                               # :131-146
        self.bad = True
        obs, self.obs = self.obs, {}
        for kf, idx in self.ordered(obs):
            kf.erase_map_point_match(idx)

    def is_in_keyframe(self, kf):
        return kf in self.obs

    def replace(self, other):                                             # :154-187, without ComputeDistinctiveDescriptors
        if other.id == self.id:
            return
        obs, self.obs, self.bad = self.obs, {}, True
        nvisible, nfound, self.replaced = self.visible, self.found, other
        for kf, idx in self.ordered(obs):
            if not other.is_in_keyframe(kf):
                kf.replace_map_point_match(idx, other)
                other.add_observation(kf, idx)
            else:
                kf.erase_map_point_match(idx)
        other.found += nfound
        other.visible += nvisible


class KeyFrame:
    def __init__(self, k, n, uright):
        self.k, self.n, self.uright, self.slots = k, n, uright, []

    def add_map_point(self, mp, idx):                                     # src/KeyFrame.cc:185-187
        self.slots[idx] = mp

    def erase_map_point_match(self, idx):                                 # :189-191
        self.slots[idx] = None

    def replace_map_point_match(self, idx, mp):                           # :195-197
        self.slots[idx] = mp

    def set_bad_flag_points(self):                                        # :362-368, the point loop, on the live vector
        for i in range(self.n):
            if self.slots[i] is not None:
                self.slots[i].erase_observation(self)


def apply_literal(state, ops):
    """The log on objects, statement by statement; returns the state on exit in the array form (obs ascending by keyframe).  For states and
    logs a host-memory call accepts, with no point too long."""
    n_tab, n_pts, cap = len(state["n_kps"]), len(state["pt_flags"]), state["held_id"].shape[1]
    opt = lambda key, p, default: default if state[key] is None else int(state[key][p])
    mono = np.full(cap, -1.0)
    kfs = [KeyFrame(k, min(int(state["n_kps"][k]), cap), mono if state["uright"] is None else state["uright"][k]) for k in range(n_tab)]
    mps = [MapPoint(p, int(state["pt_flags"][p]), int(state["pt_nobs"][p]), opt("pt_found", p, 0), opt("pt_visible", p, 0)) for p in range(n_pts)]
    for kf in kfs:
        kf.slots = [None if h < 0 else mps[h] for h in state["held_id"][kf.k]]
    for mp in mps:
        mp.obs = {kfs[k]: i for k, i in state["obs"][mp.id]}
        r, q = int(state["pt_ref"][mp.id]), opt("pt_replaced", mp.id, -1)
        mp.ref, mp.replaced = None if r < 0 else kfs[r], None if q < 0 else mps[q]
    for op, a, b, c in (pad(o) for o in ops):
        if op == ADD:
            mps[a].add_observation(kfs[b], c); kfs[b].add_map_point(mps[a], c)
        elif op == ERASE:
            mps[a].erase_observation(kfs[b])
        elif op == SET_BAD:
            mps[a].set_bad_flag()
        elif op == REPLACE:
            mps[a].replace(mps[b])
        elif op == KF_ERASE:
            kfs[b].set_bad_flag_points()
    out = copy_state(state)
    wrap = lambda x: int(np.int32(np.uint32(x & 0xFFFFFFFF)))
    for kf in kfs:
        out["held_id"][kf.k] = [-1 if m is None else m.id for m in kf.slots]
    for mp in mps:
        p = mp.id
        out["obs"][p] = [(kf.k, i) for kf, i in mp.ordered()]
        out["pt_flags"][p], out["pt_nobs"][p] = mp.other_bits | (0 if mp.bad else 1), mp.nobs
        out["pt_ref"][p] = -1 if mp.ref is None else mp.ref.k
        if out["pt_found"] is not None:
            out["pt_found"][p], out["pt_visible"][p] = wrap(mp.found), wrap(mp.visible)
        if out["pt_replaced"] is not None:
            out["pt_replaced"][p] = -1 if mp.replaced is None else mp.replaced.id
    return out


def same_state(x, y):
    """Two states equal in every array and every list."""
    for k in x:
        if k == "obs":
            if [list(map(tuple, o)) for o in x[k]] != [list(map(tuple, o)) for o in y[k]]:
                return False
        elif (x[k] is None) != (y[k] is None) or (x[k] is not None and not np.array_equal(x[k], y[k])):
            return False
    return True

"""Sequential models of the cullings of LocalMapping::Run (reference src/LocalMapping.cc).

A scene is a dict over one map:
  held[k], octave[k], uright[k], depth[k]   per keyframe k, one entry per slot: the point id (None = NULL), mvKeysUn[i].octave, mvuRight[i]
                                            (>= 0: stereo) and mvDepth[i]
  kf_bad[k], not_erase[k]                   isBad() (never read by the culling) and mbNotErase
  pt_bad[p], pt_nobs[p], pt_obs[p]          isBad(), Observations() and mObservations as a list of (keyframe, keypoint index)
  origin                                    the keyframe with mnId == 0, or None        th_depth   mThDepth
  items                                     per item GetVectorCovisibleKeyFrames() of its current keyframe, in order

Two models of KeyFrameCulling (:704-759).  cull_keyframes is the array model msl_cull_keyframes is compared with: it reads the tables on
entry and carries one set from candidate to candidate, the keyframes culled so far.  cull_keyframes_literal has objects with an
observation map, slots, EraseMapPointMatch and SetBadFlag, written from :704-759, src/KeyFrame.cc:349-368 and src/MapPoint.cc:95-146.
tests/test_cull_model.py proves them equal.  cull_recent is the verdict of MapPointCulling / MapLineCulling / MapPlaneCulling (:227-301)."""
import numpy as np

KEPT, CULLED, ORIGIN, NOT_ERASE, ABSENT = 1, 2, 3, 4, 5
RATIO_FLOAT, RATIO_INT = 0, 1
RECENT_KEEP, RECENT_ERASE_BAD, RECENT_CULL_RATIO, RECENT_CULL_OBS, RECENT_RETIRE, RECENT_INVALID = range(6)
TH_OBS = 3


# ---- the array model ---------------------------------------------------------------------------------------------------------------------
def _holds(scene, k, p):
    return p in scene["held"][k]


def point_state(scene, culled, p, consistent=False):
    """(nObs, bad, the observations left) of point p once the keyframes in `culled` have had their SetBadFlag: an observation is gone iff
    its keyframe is culled and holds the point; the point is bad iff it was on entry, or an observation is gone and nObs <= 2 (nObs only
    falls, so "was <= 2 at some erasure" is "is <= 2 now").  nObs of a point that turned bad is not the reference's (later erasures do
    nothing there); nothing reads it.  consistent: the wrong shortcut of cull_keyframes' `wrong`."""
    if scene["pt_bad"][p]:
        return scene["pt_nobs"][p], True, []
    nobs, left, erased = scene["pt_nobs"][p], [], False
    for k, idx in scene["pt_obs"][p]:
        if k in culled and (consistent or _holds(scene, k, p)):
            nobs -= 2 if scene["uright"][k][idx] >= 0 else 1
            erased = True
        else:
            left.append((k, idx))
    bad = erased and nobs <= 2
    return nobs, bad, [] if bad else left


def cull_keyframes(scene, cand, wrong=None):
    """One item: per candidate (n_mps, n_redundant, n_gone, status), and the keyframes whose SetBadFlag took effect, in order.
    wrong: one of two implementations the hand-built scenes must tell from the right one -- "entry" evaluates every candidate from the
    state on entry, "consistent" takes every observation by a culled keyframe for erased without asking whether the keyframe holds the
    point."""
    n_tab, th = len(scene["held"]), np.float32(scene["th_depth"])
    culled, order, rows = set(), [], []
    for c in cand:
        if c < 0 or c >= n_tab:
            rows.append((0, 0, 0, ABSENT)); continue
        if c == scene["origin"]:
            rows.append((0, 0, 0, ORIGIN)); continue
        n_mps = n_red = n_gone = 0
        for i, p in enumerate(scene["held"][c]):
            if p is None or scene["pt_bad"][p]:
                continue
            nobs, bad, left = point_state(scene, set() if wrong == "entry" else culled, p, wrong == "consistent")
            if bad:
                n_gone += 1; continue
            d = np.float32(scene["depth"][c][i])
            if d > th or d < 0:
                continue
            n_mps += 1
            if nobs > TH_OBS:
                level = scene["octave"][c][i]
                n_red += sum(1 for k, idx in left if k != c and scene["octave"][k][idx] <= level + 1) >= TH_OBS
        redundant = float(n_red) > 0.9 * float(n_mps)
        assert redundant == (10 * n_red > 9 * n_mps)
        if redundant and not scene["not_erase"][c]:
            culled.add(c); order.append(c)
        rows.append((n_mps, n_red, n_gone, NOT_ERASE if redundant and scene["not_erase"][c] else CULLED if redundant else KEPT))
    return rows, order


def final_state(scene, culled):
    """Per point (bad, nObs or None for a bad point, the sorted observations) after the keyframes in `culled`, by the array model's rules."""
    out = []
    for p in range(len(scene["pt_bad"])):
        nobs, bad, left = point_state(scene, set(culled), p)
        out.append((bad, None if bad else nobs, sorted(left)))
    return out


# ---- the literal model -------------------------------------------------------------------------------------------------------------------
class MapPoint:
    def __init__(self, pid, bad, nobs):
        self.id, self.bad, self.nobs, self.obs = pid, bad, nobs, {}       # obs: mObservations, KeyFrame -> idx, in insertion order

    def erase_observation(self, kf):                                      # src/MapPoint.cc:95-119
        bad = False
        if kf in self.obs:
            idx = self.obs[kf]
            self.nobs -= 2 if kf.uright[idx] >= 0 else 1
            del self.obs[kf]
            if self.nobs <= 2:
                bad = True
        if bad:
            self.set_bad_flag()

    def set_bad_flag(self):                                               # :131-146
        self.bad = True
        obs, self.obs = self.obs, {}
        for kf, idx in obs.items():
            kf.erase_map_point_match(idx)


class KeyFrame:
    def __init__(self, k, scene, points):
        self.k, self.is_origin, self.not_erase = k, k == scene["origin"], scene["not_erase"][k]
        self.slots = [None if p is None else points[p] for p in scene["held"][k]]
        self.entry = list(self.slots)
        self.octave, self.uright, self.depth = scene["octave"][k], scene["uright"][k], scene["depth"][k]
        self.set_bad = False                                              # SetBadFlag got past its two returns

    def erase_map_point_match(self, idx):
        self.slots[idx] = None

    def set_bad_flag(self):                                               # src/KeyFrame.cc:349-368, the point loop
        if self.is_origin or self.not_erase:
            return
        self.set_bad = True
        for mp in self.slots:                                             # the live vector: a point that turns bad NULLs other keyframes' slots
            if mp is not None:
                mp.erase_observation(self)


def build_objects(scene):
    """The map as objects.  A point that is bad on entry has no observations (SetBadFlag and Replace clear them)."""
    points = [MapPoint(p, b, n) for p, (b, n) in enumerate(zip(scene["pt_bad"], scene["pt_nobs"]))]
    kfs = [KeyFrame(k, scene, points) for k in range(len(scene["held"]))]
    for mp in points:
        if not mp.bad:
            for k, idx in scene["pt_obs"][mp.id]:
                mp.obs[kfs[k]] = idx
    return kfs, points


def object_state(points):
    """Per point (bad, nObs, the sorted observations)."""
    return [(mp.bad, mp.nobs, sorted((kf.k, idx) for kf, idx in mp.obs.items())) for mp in points]


def cull_keyframes_literal(scene, cand):
    """LocalMapping::KeyFrameCulling over objects: the rows and the order of cull_keyframes, and the state of every point afterwards."""
    kfs, points = build_objects(scene)
    th, rows, order = np.float32(scene["th_depth"]), [], []
    for c in cand:
        kf = kfs[c]
        if kf.is_origin:                                                  # :715
            rows.append((0, 0, 0, ORIGIN)); continue
        vp = list(kf.slots)
        n_red = n_mps = 0
        for i, mp in enumerate(vp):
            if mp is not None and not mp.bad:
                if np.float32(kf.depth[i]) > th or np.float32(kf.depth[i]) < 0:
                    continue
                n_mps += 1
                if mp.nobs > TH_OBS:
                    level, n = kf.octave[i], 0
                    for kfi, idx in dict(mp.obs).items():
                        if kfi is kf:
                            continue
                        if kfi.octave[idx] <= level + 1:
                            n += 1
                            if n >= TH_OBS:
                                break
                    if n >= TH_OBS:
                        n_red += 1
        n_gone = sum(1 for mp in kf.entry if mp is not None and not scene["pt_bad"][mp.id] and mp.bad)
        redundant = n_red > 0.9 * n_mps
        if redundant:
            kf.set_bad = False
            kf.set_bad_flag()
            if kf.set_bad:
                order.append(c)
        rows.append((n_mps, n_red, n_gone, KEPT if not redundant else CULLED if kf.set_bad else NOT_ERASE))
    return rows, order, object_state(points)


def replay(scene, culled):
    """KeyFrame::SetBadFlag on the keyframes msl_cull_keyframes reports as culled, in order, over fresh objects: what the caller does with
    the result.  Returns the state of every point."""
    kfs, points = build_objects(scene)
    for c in culled:
        kfs[c].set_bad_flag()
    return object_state(points)


# ---- the recent elements -----------------------------------------------------------------------------------------------------------------
def cull_recent(found, visible, first_kf_id, nobs, live, cur_kf_id, th_obs, ratio_form):
    """The branch MapPointCulling / MapPlaneCulling (RATIO_FLOAT) or MapLineCulling (RATIO_INT) takes for one element."""
    if not live:
        return RECENT_ERASE_BAD
    if ratio_form == RATIO_INT:
        if visible == 0:
            return RECENT_INVALID                                         # the reference divides by zero
        q = abs(int(found)) // abs(int(visible))                          # C division truncates toward zero
        ratio = np.float32(-q if (found < 0) != (visible < 0) else q)
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.float32(found) / np.float32(visible)
    age = int(np.int32(cur_kf_id) - np.int32(first_kf_id))
    if ratio < np.float32(0.25):
        return RECENT_CULL_RATIO
    if age >= 2 and nobs <= th_obs:
        return RECENT_CULL_OBS
    if age >= 3:
        return RECENT_RETIRE
    return RECENT_KEEP

"""Fixed-seed inputs for msl_refresh_map_points / msl_covisibility.
  graph(name)        a keyframe graph of tests/fuse_scenes.py after a literal SearchInNeighbors, with two bad keyframes and a reference
                     keyframe per point (sometimes one that no longer observes the point)
  Scene              keyframes around the origin; every observation of a point is a keypoint of its own in the observing keyframe (a
                     descriptor within some bits of the point's, a random octave), the observations in a random (not ascending) order
  counts / special / batch / lines / covis_*   the scenes of tests/test_mappoint_gpu.py, built once and shared with their model results
Descriptors of one point lie within 40 bits of each other, so medians differ and ties happen only where they are built."""
import functools

import numpy as np

from tests import fuse_model as fm
from tests import fuse_scenes as fs
from tests import mappoint_model as mm
from tests.triangulate_scenes import KP, desc_flip, make_pose

F32 = np.float32
COUNTS = (1, 2, 3, 4, 5, 63, 64, 65, 128, 255, 256, 257)


def graph(name, seed=5):
    """(graph, prm): fuse_scenes.graph(name) after the literal SearchInNeighbors; keyframes 8 and 4 bad; ref of a point = one of its
    observers (4 in 5) or any keyframe."""
    g, p, cur, targets = fs.graph(name)
    fm.search_in_neighbors_literal(g, p, cur, targets)
    r = np.random.RandomState(seed)
    g.kfs[8].bad = True; g.kfs[4].bad = True
    for mp in g.mps:
        ks = sorted(mp.obs)
        mp.ref = int(ks[r.randint(len(ks))]) if ks and r.uniform() < 0.8 else int(r.randint(len(g.kfs)))
    return g, mm.params()


class Scene:
    def __init__(self, seed, n_tab, nlevels=8):
        self.r = r = np.random.RandomState(seed)
        self.prm = mm.params(nlevels)
        self.poses = [make_pose(r.uniform(-1, 1, 3) * (0.8, 0.3, 0.5), r.uniform(-0.1, 0.1, 3)) for _ in range(n_tab)]
        self.feats = [[] for _ in range(n_tab)]
        self.obs, self.xyz, self.flags, self.ref, self.tags = [], [], [], [], {}

    def keypoint(self, k, desc, octave=None):
        self.feats[k].append((desc, self.r.randint(0, self.prm["nlevels"]) if octave is None else octave))
        return len(self.feats[k]) - 1

    def point(self, kfs, xyz=None, descs=None, ref="random", octave=None, bad=False, tag=None, flips=20):
        """A point observed by the keyframes kfs, in that order.  descs: the descriptor of every observation (default: within `flips`
        bits of a random one); ref: a keyframe, "random" (one of kfs) or "absent"; octave: of the reference keypoint."""
        r = self.r
        base = r.randint(0, 256, 32).astype(np.uint8)
        if ref == "random":
            ref = int(kfs[r.randint(len(kfs))]) if len(kfs) else 0
        elif ref == "absent":
            ref = next(k for k in range(len(self.poses)) if k not in kfs)
        obs = []
        for n, k in enumerate(kfs):
            d = np.asarray(descs[n], np.uint8) if descs is not None else desc_flip(base, r, r.randint(0, flips + 1))
            obs.append((int(k), self.keypoint(k, d, octave if k == ref else None)))
        z = r.uniform(2, 6)
        self.obs.append(obs)
        self.xyz.append(np.asarray(xyz, F32) if xyz is not None else np.array([r.uniform(-0.6, 0.6) * z, r.uniform(-0.4, 0.4) * z, z], F32))
        self.flags.append(0 if bad else 1); self.ref.append(ref)
        if tag:
            self.tags[tag] = len(self.obs) - 1
        return len(self.obs) - 1

    def random_point(self, n, **kw):
        return self.point(self.r.permutation(len(self.poses))[:n].tolist(), **kw)

    def finish(self, bad_kfs=(), geometry=True):
        table = []
        for k, fl in enumerate(self.feats):
            t = dict(desc=np.array([d for d, _ in fl], np.uint8).reshape(len(fl), 32), bad=k in bad_kfs)
            if geometry:
                kp = np.zeros(len(fl), KP)
                kp["octave"] = [o for _, o in fl]; kp["size"] = 31.0; kp["class_id"] = -1
                t.update(kps_un=kp, Tcw=self.poses[k])
            table.append(t)
        points = dict(flags=np.array(self.flags, np.uint8))
        if geometry:
            points.update(xyz=np.array(self.xyz, F32).reshape(-1, 3), ref=np.array(self.ref, np.int32))
        return dict(prm=self.prm, table=table, obs=self.obs, points=points, tags=dict(self.tags), n_pts=len(self.obs))


def with_model(s, ids=None, what=3):
    """The scene with ids and the model's result (computed once; nobody changes it)."""
    ids = list(range(s["n_pts"])) if ids is None else ids
    return dict(s, ids=ids, what=what, want=mm.refresh_map_points(s["prm"], s["table"], s["obs"], s["points"], ids, what, select=mm.select_descriptor_fast))


@functools.lru_cache(None)
def counts():
    """One point per observation count of COUNTS over 260 keyframes, tagged n<count>."""
    S = Scene(11, 260)
    for n in COUNTS:
        S.random_point(n, tag="n%d" % n, flips=40)
    return with_model(S.finish())


@functools.lru_cache(None)
def special():
    """Ties, bad keyframes (2 and 5), a bad point, a point without observations, the reference keyframe's place, octaves out of range, a
    point at a camera centre."""
    S = Scene(12, 9)
    S.poses[0] = make_pose((0.0, 0.0, 0.0))                            # its camera centre is exactly the origin
    r = S.r
    a = r.randint(0, 256, 32).astype(np.uint8)
    near = desc_flip(a, r, 2)                                          # b, c, d within 2 .. 4 bits of each other, a far from all
    far = (~a).astype(np.uint8)
    S.point([1, 3, 4, 6], descs=[far, near, desc_flip(near, r, 2), desc_flip(near, r, 2)], tag="tie_later_rows")   # rows 1 .. 3 tie: 1 wins
    S.point([6, 4, 3, 1, 7], descs=[a] * 5, tag="all_equal")
    S.point([3, 1, 4], descs=[a, desc_flip(a, r, 4), desc_flip(a, r, 4)], tag="tie_three")
    S.point([2, 1, 5, 3, 4, 6], tag="bad_mixed", ref=2)                # bad keyframes first and in the middle: best_obs skips them
    S.point([2, 7], descs=[a, far], tag="bad_first_of_two", ref=7)     # N = 1 after the filter: position 1
    S.point([5, 2], tag="all_bad", ref=5)
    S.point([1, 3, 4], bad=True, tag="bad_point")
    S.point([], tag="no_obs")
    S.point([1, 3, 4, 6, 7], ref=1, tag="ref_first")
    S.point([1, 3, 4, 6, 7], ref=4, tag="ref_middle")
    S.point([1, 3, 4, 6, 7], ref=7, tag="ref_last")
    S.point([1, 3, 4], ref="absent", tag="ref_absent")                 # keyframe 0: its keypoint 0
    S.point([1, 3, 4], ref=3, octave=8, tag="octave_high")
    S.point([1, 3, 4], ref=3, octave=-1, tag="octave_negative")
    S.point([0, 3], xyz=(0.0, 0.0, 0.0), ref=3, tag="at_centre")       # normali = 0 for keyframe 0: a NaN normal, finite distances
    S.point([3, 0], xyz=(0.0, 0.0, 0.0), ref=0, tag="at_ref_centre")   # and distances 0
    return with_model(S.finish(bad_kfs=(2, 5)))


@functools.lru_cache(None)
def batch(n_items=5000, n_tab=40, seed=13):
    """n_items points with 1 .. 12 observations, among them as many again that are not named; the ids in a shuffled order."""
    S = Scene(seed, n_tab)
    for _ in range(2 * n_items):
        S.random_point(S.r.randint(1, 13))
    s = S.finish(bad_kfs=(7,))
    return with_model(s, S.r.permutation(2 * n_items)[:n_items].tolist())


@functools.lru_cache(None)
def lines():
    """A line-descriptor table only (no keypoints, poses, positions or reference keyframes): MSL_REFRESH_DESC alone."""
    S = Scene(14, 12)
    for _ in range(150):
        S.random_point(S.r.randint(1, 9))
    S.point([], tag="no_obs")
    return with_model(S.finish(bad_kfs=(3,), geometry=False), what=mm.REFRESH_DESC)


def _held(S, kf_points):
    """held_id per keyframe from {keyframe: [point id per slot]} (msl_covisibility reads no keypoint: the slots are all there is)."""
    t = S.finish()
    for k, kf in enumerate(t["table"]):
        kf["held_id"] = np.array(kf_points.get(k, []), np.int32)
    return t


@functools.lru_cache(None)
def covis_crafted():
    """Keyframe 0 holds 60 points; the weights it gives: keyframes 1, 2, 3 -> 14, 15, 16; 4 and 5 -> 20 each (a tie); 6 -> 15;
    itself (skipped); slots with a bad point, an id outside the table, -1, and one point in two slots.  Keyframe 7 holds points that give
    8 and 9 the weight 3 each and 10 the weight 2 (none reaches 15: the lowest index of the maxima); keyframe 11 holds nothing it shares."""
    S = Scene(15, 12)
    want = {1: 14, 2: 15, 3: 16, 4: 20, 5: 20, 6: 15}
    held0 = []
    for i in range(20):
        held0.append(S.point([0] + [k for k, w in want.items() if i < w]))
    twice = S.point([0, 9])
    bad = S.point([0, 1, 2, 3], bad=True)
    held0 += [twice, -1, bad, 10 ** 6, twice]
    held7 = [S.point([7, 8, 9, 10]), S.point([8, 9, 10, 7]), S.point([9, 8])]
    held11 = [S.point([11]), -1]
    t = _held(S, {0: held0, 7: held7, 11: held11})
    t["kfs"] = [0, 7, 11, 4]
    return t


@functools.lru_cache(None)
def covis_random(n_tab=30, n_pts=900, seed=16):
    """Every keyframe holds the points that observe it (slot = the observation's keypoint), 5 % of the points bad."""
    S = Scene(seed, n_tab)
    for _ in range(n_pts):
        S.random_point(S.r.randint(1, 20), bad=S.r.uniform() < 0.05)
    t = S.finish()
    for k, kf in enumerate(t["table"]):
        kf["held_id"] = np.full(len(kf["desc"]), -1, np.int32)
    for pid, obs in enumerate(t["obs"]):
        for k, i in obs:
            t["table"][k]["held_id"][i] = pid
    t["kfs"] = list(range(n_tab))
    return t


@functools.lru_cache(None)
def covis_wide(n_tab=4096):
    """n_tab = 4096 with 6 keypoints per keyframe: the observers of keyframe 9's points are spread over the whole table."""
    S = Scene(17, n_tab)
    held = {9: [S.point([9] + S.r.choice(np.setdiff1d(np.arange(n_tab), [9]), 40, replace=False).tolist()) for _ in range(6)],
            4095: [S.point([4095, 0, 4094]), S.point([0, 4095])]}
    t = _held(S, held)
    t["kfs"] = [9, 4095, 100]
    return t

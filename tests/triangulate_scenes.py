"""Fixed scenes for msl_triangulate_new_points: 3-D points seen from a few keyframes with known poses at 160 x 120-scale intrinsics, built
from tracks (one 3-D point per view, so a false match is a track whose views see different points).  Descriptors are random with a few
flipped bits per view, node ids are the scene's (no vocabulary), stereo and mono keypoints are mixed, and raw_xy differs from kps_un by a
distortion offset.  scene(name) -> dict(table, items, prm, what); model(name) -> the sequential model's result per item
(tests/triangulate_model.py), computed once and shared.  Seeds are chosen so that tests/test_triangulate_model.py::test_margins holds."""
import functools

import numpy as np

from tests import triangulate_model as tm

F32 = np.float32
KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
FX, FY, CX, CY, BF = 100.0, 100.0, 79.5, 59.5, 8.0                       # b = 0.08 m


def prm(**kw):
    return tm.params(FX, FY, CX, CY, BF, **kw)


def make_pose(centre, rvec=(0.0, 0.0, 0.0)):
    """Rows 0-2 of a CV_32F Tcw for a camera at `centre` (world) with orientation Rwc = exp(rvec)."""
    w = np.asarray(rvec, float); th = np.linalg.norm(w)
    Rwc = np.eye(3)
    if th > 0:
        k = w / th; K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        Rwc = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    Rcw = Rwc.T
    return np.concatenate([Rcw, (-Rcw @ np.asarray(centre, float))[:, None]], 1).astype(F32)


class Builder:
    """Keyframes as lists of features; finish() permutes every keyframe's features (so idx1 != idx2 for a track) and packs the arrays."""

    def __init__(self, seed, poses):
        self.r = np.random.RandomState(seed)
        self.poses = [np.asarray(p, F32) for p in poses]
        self.feats = [[] for _ in poses]
        self.next_node = 0

    def project(self, k, X):
        T = self.poses[k].astype(float)
        Xc = T[:, :3] @ np.asarray(X, float) + T[:, 3]
        return FX * Xc[0] / Xc[2] + CX, FY * Xc[1] / Xc[2] + CY, Xc[2]

    def track(self, X, views, stereo=0.6, octave=None, node=None, flips=6, held=(), rot=None, noise=0.25, angle=None, ur_depth=None, desc=None,
              depth_noise=0.0, tag=None):
        """One descriptor seen in `views` (keyframe indices).  X: a world point, or {view: point}; stereo: probability, or {view: bool};
        octave: int or {view: int}; rot {view: degrees subtracted from the angle in that view}; ur_depth {view: depth uright is built from}."""
        r = self.r
        base = r.randint(0, 256, 32).astype(np.uint8) if desc is None else desc
        node = r.randint(0, 12) if node is None else node
        angle = r.uniform(0, 360) if angle is None else angle
        o0 = r.randint(0, 4)
        for k in views:
            Xk = X[k] if isinstance(X, dict) else X
            u, v, z = self.project(k, Xk)
            u += r.normal(0, noise); v += r.normal(0, noise)
            st = stereo[k] if isinstance(stereo, dict) else (r.uniform() < stereo)
            d = desc_flip(base, r, r.randint(0, flips + 1))
            o = octave[k] if isinstance(octave, dict) else (o0 if octave is None else octave)
            a = (angle - (rot or {}).get(k, 0.0) + r.uniform(-2, 2)) % 360.0
            zs = (ur_depth or {}).get(k, z) * (1 + r.normal(0, depth_noise))
            self.feats[k].append(dict(x=u, y=v, raw=(u + 0.9 + 0.01 * (u - CX), v - 0.6 + 0.01 * (v - CY)), ur=(u - BF / zs) if st else -1.0,
                                      depth=zs if st else -1.0, desc=d, node=node, held=1 if k in held else 0, octave=o, angle=a, tag=tag))
        return base

    def clutter(self, k, n, node_range=(0, 16)):
        r = self.r
        for _ in range(n):
            st = r.uniform() < 0.5
            z = r.uniform(1, 6)
            u = r.uniform(0, 160)
            self.feats[k].append(dict(x=u, y=r.uniform(0, 120), raw=(u + 1, 0), ur=(u - BF / z) if st else -1.0, depth=z if st else -1.0,
                                      desc=r.randint(0, 256, 32).astype(np.uint8), node=r.randint(*node_range) if r.uniform() < 0.85 else -1,
                                      held=int(r.uniform() < 0.2), octave=r.randint(0, 8), angle=r.uniform(0, 360), tag=None))

    def finish(self, shuffle=True):
        table = []
        for k, fl in enumerate(self.feats):
            order = self.r.permutation(len(fl)) if shuffle else np.arange(len(fl))
            fl = [fl[i] for i in order]
            n = len(fl)
            kp = np.zeros(n, KP)
            kp["x"] = [f["x"] for f in fl]; kp["y"] = [f["y"] for f in fl]; kp["size"] = 31.0; kp["angle"] = [f["angle"] for f in fl]
            kp["octave"] = [f["octave"] for f in fl]; kp["class_id"] = -1
            table.append(dict(kps_un=kp, raw_xy=np.array([f["raw"] for f in fl], F32).reshape(n, 2), uright=np.array([f["ur"] for f in fl], F32),
                              depth=np.array([f["depth"] for f in fl], F32), desc=np.array([f["desc"] for f in fl], np.uint8).reshape(n, 32),
                              node=np.array([f["node"] for f in fl], np.int32), held=np.array([f["held"] for f in fl], np.uint8),
                              Tcw=self.poses[k], tags=[f["tag"] for f in fl]))
        return table


def desc_flip(base, r, nbits):
    d = base.copy()
    for b in r.choice(256, nbits, replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def _points(r, n, zlo=2.0, zhi=6.0, spread=0.55):
    z = r.uniform(zlo, zhi, n)
    return np.stack([r.uniform(-spread, spread, n) * z, r.uniform(-spread * 0.7, spread * 0.7, n) * z, z], 1)


def _general(seed, n_kf=4, n_pts=60, clutter=15, check_orientation=False, only_stereo=False):
    """Keyframes side by side with small rotations; every point seen by a random subset of at least two."""
    r = np.random.RandomState(seed)
    poses = [make_pose((0.35 * k + r.uniform(-0.05, 0.05), r.uniform(-0.08, 0.08), r.uniform(-0.1, 0.1)), r.uniform(-0.06, 0.06, 3)) for k in range(n_kf)]
    B = Builder(seed + 1, poses)
    for X in _points(r, n_pts):
        views = [k for k in range(n_kf) if r.uniform() < 0.75]
        if len(views) < 2:
            views = [0, 1 + r.randint(n_kf - 1)]
        held = [k for k in views if r.uniform() < 0.12]
        rot = {k: (0.0 if r.uniform() < 0.7 else r.choice([90.0, 180.0, 270.0])) for k in views} if check_orientation else None
        B.track(X, views, held=held, rot=rot)
    for k in range(n_kf):
        B.clutter(k, clutter)
    return B


def _scene_general(seed, **kw):
    B = _general(seed, **kw)
    n = len(B.poses)
    table = B.finish()
    return dict(table=table, items=[(0, list(range(1, n))), (n - 1, list(range(n - 2, -1, -1)))],
                prm=prm(check_orientation=kw.get("check_orientation", False), only_stereo=kw.get("only_stereo", False)), what="general")


def _scene_special():
    """Everything a generic scene does not reach: a neighbour skipped for its baseline, a forward-moving neighbour (epipole in the image: the
    epipole rejection, UnprojectStereo of either side, low parallax), points behind a camera, stereo inconsistencies, a scale mismatch,
    descriptor duplicates on either side (a tie; two idx1 with one idx2), nodes on one side only and node = -1."""
    r = np.random.RandomState(77)
    # 0: KF1; 1: too close (skipped); 2: behind KF1 on its axis; 3: to the side; 4: in front of KF1 on its axis
    poses = [make_pose((0, 0, 0)), make_pose((0.02, 0.01, 0.0)), make_pose((0.01, 0.0, -0.45)), make_pose((0.4, 0.02, 0.0), (0, -0.05, 0)),
             make_pose((0.0, 0.01, 0.5))]
    B = Builder(78, poses)
    for X in _points(r, 30):
        B.track(X, [0, 1, 2, 3])
    # near the axis, seen from 0 and 2 (forward motion): ray parallax below the stereo parallax
    for i in range(10):
        ang = r.uniform(0, 2 * np.pi); rad = r.uniform(0.13, 0.2); z = r.uniform(2.0, 3.0)
        if i % 4 == 2:                                                    # mono in both: keep the ray parallax below acos(0.9998)
            rad = r.uniform(0.13, 0.17); z = r.uniform(4.2, 5.0)
        st = [dict([(0, True), (2, False)]), dict([(0, False), (2, True)]), dict([(0, False), (2, False)]), dict([(0, True), (2, True)])][i % 4]
        B.track((rad * z * np.cos(ang), rad * z * np.sin(ang), z), [0, 2], stereo=st, node=20 + i % 3, octave=0, tag="axis%d" % (i % 4), noise=0.05)
    # mono in both, a few pixels from the epipole of keyframe 2
    for i in range(3):
        B.track((0.02 * (i + 1), 0.015, 2.5), [0, 2], stereo={0: False, 2: False}, node=24, octave=1, tag="epipole", noise=0.05)
    # behind KF1, in front of keyframe 2 (mono): z1 <= 0
    for i in range(3):
        ray = np.array([0.1 * (i + 1), 0.05, 1.0])
        B.track({0: 2.0 * ray, 2: -0.25 * ray}, [0, 2], stereo={0: False, 2: False}, node=25, octave=0, tag="z1", noise=0.0)
    # a stereo point of KF1 0.35 m ahead of it, behind keyframe 4: UnprojectStereo of KF1, then z2 <= 0
    for i in range(3):
        B.track((0.02 * (i + 1), 0.01, 0.35), [0, 4], stereo={0: True, 4: False}, node=26, octave=0, tag="z2", noise=0.0)
    # stereo in KF1 whose depth disagrees with the point keyframe 3 sees on the same ray: reprojection error 1 (in uright)
    for i in range(3):
        ray = np.array([0.1 * i - 0.1, 0.04, 1.0])
        B.track({0: 1.5 * ray, 3: 6.0 * ray}, [0, 3], stereo={0: True, 3: False}, node=27, octave=0, tag="reproj1", noise=0.0)
    # mono in KF1, stereo in keyframe 3 with uright built from a wrong depth: reprojection error 2
    for i in range(3):
        X = np.array([0.3 * i - 0.2, 0.1, 2.0])
        B.track(X, [0, 3], stereo={0: False, 3: True}, ur_depth={3: 20.0}, node=28, octave=0, tag="reproj2", noise=0.0)
    # octave 5 against octave 0 at equal distances: scale consistency
    for i in range(3):
        B.track((0.4 * i - 0.3, -0.2, 3.0), [0, 3], octave={0: 5, 3: 0}, node=29, tag="scale", noise=0.0)
    # far away and mono in both: low parallax
    for i in range(3):
        B.track((3.0 * i - 2.0, 1.0, 40.0 + 5 * i), [0, 3], stereo={0: False, 3: False}, node=30, octave=2, tag="far", noise=0.05)
    # the same descriptor twice in keyframe 3 (a tie) and twice in KF1 (two idx1, one idx2)
    for i in range(3):
        X = np.array([0.5 * i - 0.4, 0.3, 3.5])
        d = B.track(X, [0], stereo={0: True}, node=31, flips=0, octave=1, tag="tie1", noise=0.0)
        B.track(X, [3], stereo={3: True}, node=31, flips=0, octave=1, desc=d, tag="tie2a", noise=0.0)
        B.track(X, [3], stereo={3: True}, node=31, flips=0, octave=1, desc=d, tag="tie2b", noise=0.0)
        X = np.array([0.5 * i - 0.4, -0.5, 3.0])
        d = B.track(X, [3], stereo={3: True}, node=32, flips=0, octave=1, tag="share2", noise=0.0)
        B.track(X, [0], stereo={0: True}, node=32, flips=0, octave=1, desc=d, tag="share1a", noise=0.0)
        B.track(X, [0], stereo={0: True}, node=32, flips=0, octave=1, desc=d, tag="share1b", noise=0.0)
    # nodes present on one side only, and features in no list
    for i in range(4):
        X = _points(r, 1)[0]
        d = B.track(X, [0], node=40 + i, tag="only1")
        B.track(X, [3], node=50 + i, desc=d, tag="only2")
        d = B.track(_points(r, 1)[0], [0, 3], node=-1, tag="nolist")
    for k in range(5):
        B.clutter(k, 10)
    table = B.finish()
    return dict(table=table, items=[(0, [1, 2, 3, 4]), (3, [0, 2])], prm=prm(), what=_scene_special.__doc__)


def _scene_chain():
    """KF1 = 0 with neighbours 1 and 2, orientation check on.  In neighbour 2 the candidates rotate by 0 (6 points, 4 of them also seen by
    neighbour 1 and created there), 90 (5), 180 (4) and 270 degrees (3): with the chain the kept bins are 3, 6, 9, without it 0, 3, 6."""
    r = np.random.RandomState(5)
    poses = [make_pose((0, 0, 0)), make_pose((0.35, 0.0, 0.02), (0.0, -0.03, 0.0)), make_pose((-0.3, 0.03, 0.0), (0.0, 0.04, 0.0))]
    B = Builder(6, poses)
    pts = _points(r, 18, 2.5, 4.0, 0.4)
    for i, X in enumerate(pts):
        grp = 0 if i < 6 else 1 if i < 11 else 2 if i < 15 else 3
        views = [0, 1, 2] if i < 4 else [0, 2]
        B.track(X, views, stereo=1.0, rot={2: 90.0 * grp}, node=i % 5, octave=1, flips=3, tag="g%d" % grp)
    table = B.finish()
    return dict(table=table, items=[(0, [1, 2]), (0, [2])], prm=prm(check_orientation=True), what=_scene_chain.__doc__)


def _scene_ring():
    """Seventeen small keyframes on an arc, for items with 10 and 16 neighbours."""
    r = np.random.RandomState(31)
    n_kf = 17
    poses = [make_pose((0.15 * k, 0.03 * np.sin(k), 0.02 * np.cos(2 * k)), (0.0, -0.01 * k, 0.0)) for k in range(n_kf)]
    B = Builder(32, poses)
    for X in _points(r, 70, 2.0, 5.0, 0.35) + np.array([1.2, 0, 0]):
        views = [k for k in range(n_kf) if r.uniform() < 0.45]
        if len(views) >= 2:
            B.track(X, views, held=[k for k in views if r.uniform() < 0.1])
    for k in range(n_kf):
        B.clutter(k, 4)
    table = B.finish()
    return dict(table=table, items=[(8, [7, 9, 6, 10, 5, 11, 4, 12, 3, 13]), (0, list(range(1, 17)))], prm=prm(), what=_scene_ring.__doc__)


SCENES = dict(general=lambda: _scene_general(101), orient=lambda: _scene_general(202, n_kf=5, n_pts=90, check_orientation=True),
              stereo_only=lambda: _scene_general(303, n_kf=3, only_stereo=True), big=lambda: _scene_general(404, n_kf=6, n_pts=170, clutter=30),
              special=_scene_special, chain=_scene_chain, ring=_scene_ring)
ALL = tuple(SCENES)


@functools.lru_cache(None)
def scene(name):
    return SCENES[name]()


@functools.lru_cache(None)
def model(name):
    """[create_new_map_points result per item], with the margins of every decision in model_margins(name)."""
    s = scene(name)
    margins = []
    res = [tm.create_new_map_points(s["prm"], s["table"], c, nb, margins=margins) for c, nb in s["items"]]
    _MARGINS[name] = margins
    return res


_MARGINS = {}


def model_margins(name):
    model(name)
    return _MARGINS[name]


def limit_scene():
    """cap = 8192: one pair with n = 8192 in both keyframes, nodes of at most 64 features and one node of 1024.  Every feature of KF1 is a
    point seen by both; the positions are exact (no noise), descriptors within 8 bits."""
    r = np.random.RandomState(9)
    n = 8192
    poses = [make_pose((0, 0, 0)), make_pose((0.4, 0.02, 0.05), (0.01, -0.04, 0.0))]
    B = Builder(10, poses)
    pts = _points(r, n, 2.0, 7.0, 0.6)
    for i, X in enumerate(pts):
        node = 0 if i < 1024 else 1 + (i - 1024) // 64 + 1000 * ((i - 1024) % 3 == 0)
        B.track(X, [0, 1], node=node, flips=4, noise=0.1, held=[k for k in (0, 1) if r.uniform() < 0.05])
    return dict(table=B.finish(), items=[(0, [1])], prm=prm(check_orientation=True), what=limit_scene.__doc__)


def combine(names):
    """The tables of several scenes as one table, with their items re-indexed: (table, items, [(name, item index in the scene)])."""
    table, items, origin = [], [], []
    for nme in names:
        s = scene(nme)
        off = len(table)
        table += s["table"]
        for q, (c, nb) in enumerate(s["items"]):
            items.append((c + off, [k + off for k in nb])); origin.append((nme, q))
    return table, items, origin

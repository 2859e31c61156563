"""Sequential CPU models of what LocalMapping runs on its map points and keyframe right after the fusion: MapPoint::
ComputeDistinctiveDescriptors (reference src/MapPoint.cc:210-270), MapPoint::UpdateNormalAndDepth (:282-322) and the counting and ordering
of KeyFrame::UpdateConnections (src/KeyFrame.cc:230-299), in two forms:

  refresh_map_points / covisibility      what msl_refresh_map_points / msl_covisibility compute, on the arrays they take (observations as
                                         lists per point id, in the caller's order)
  compute_distinctive_descriptors,       the reference's statements in their order on the object graph of tests/fuse_model.py (Graph,
  update_normal_and_depth,               MapPoint with its observation map, KeyFrame with its slots), with a bad flag per keyframe and a
  update_connections                     reference keyframe per point added here (attributes `bad` of a KeyFrame, `ref` of a MapPoint)

Test infrastructure only.  Float conventions as tests/triangulate_model.py.  std::map<KeyFrame*, size_t> iterates in
pointer order in the reference; the literal form iterates in keyframe id order (= creation order), the array form in the order given."""
import math

import numpy as np

from tests import local_match_model as lm
from tests.fuse_model import hamming

F32 = np.float32
REFRESH_DESC, REFRESH_NORMAL = 1, 2
DESC_WRITTEN, NORMAL_WRITTEN, BAD, NO_OBS, NO_LIVE_KF, TOO_MANY, BAD_OCTAVE = 1, 2, 4, 8, 16, 32, 64
BITS = ("DESC_WRITTEN", "NORMAL_WRITTEN", "BAD", "NO_OBS", "NO_LIVE_KF", "TOO_MANY", "BAD_OCTAVE")
OBS_MAX = 256


def params(nlevels=8, scale_factor=1.2):
    sf = np.ones(nlevels, F32)
    for i in range(1, nlevels):
        sf[i] = sf[i - 1] * F32(scale_factor)
    return dict(nlevels=nlevels, scale_factors=sf)


def select_descriptor(descs):
    """src/MapPoint.cc:239-264 on a list of 32-byte rows: (BestIdx, BestMedian)."""
    N = len(descs)
    D = np.zeros((N, N), np.int64)
    for i in range(N):
        for j in range(i + 1, N):
            D[i, j] = D[j, i] = hamming(descs[i], descs[j])
    best_median, best = 2 ** 31 - 1, 0
    for i in range(N):
        median = int(np.sort(D[i])[int(0.5 * (N - 1))])
        if median < best_median:
            best_median, best = median, i
    return best, best_median


def select_descriptor_fast(descs):
    """select_descriptor with the distance matrix by numpy (the same integers): for the large observation counts of the GPU tests."""
    bits = np.unpackbits(np.asarray(descs, np.uint8).reshape(len(descs), 32), axis=1).astype(np.int32)
    D = bits @ (1 - bits).T
    D = D + D.T
    med = np.sort(D, axis=1)[:, int(0.5 * (len(descs) - 1))]
    best = int(np.argmin(med))                                        # the first minimum: strict <
    return best, int(med[best])


def camera_centre(Tcw):
    T = np.asarray(Tcw, F32).reshape(3, 4)
    return lm.gemm3(T, True, -1.0, T[:, 3])                            # KeyFrame::SetPose: Ow = -Rwc * tcw


def view_vector(Ow, xyz):
    """(xyz - Ow in float, cv::norm of it: the square root of a double sum)."""
    v = np.asarray(xyz, F32) - Ow
    return v, math.sqrt(sum(float(v[a]) * float(v[a]) for a in range(3)))


def normal_and_depth(prm, centres, ref_centre, level, xyz):
    """src/MapPoint.cc:299-321 for the observing keyframes' camera centres in list order: (normal, (min, max))."""
    acc = np.zeros(3, F32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for Ow in centres:
            v, nrm = view_vector(Ow, xyz)
            inv = np.float64(1.0) / np.float64(nrm)
            for a in range(3):
                acc[a] = acc[a] + F32(np.float64(v[a]) * inv)
        inv_n = 1.0 / len(centres)
        normal = np.array([F32(np.float64(acc[a]) * inv_n) for a in range(3)], F32)
        _, d = view_vector(ref_centre, xyz)
        dmax = F32(d) * F32(prm["scale_factors"][level])
        dmin = dmax / F32(prm["scale_factors"][prm["nlevels"] - 1])
    return normal, np.array([dmin, dmax], F32)


def refresh_map_points(prm, table, observations, points, ids, what=REFRESH_DESC | REFRESH_NORMAL, select=select_descriptor):
    """msl_refresh_map_points.  table: keyframe dicts (desc; kps_un, Tcw; bad); observations[id] = [(keyframe, keypoint), ...]; points:
    dict(flags, xyz, ref).  Returns the per-item outputs as arrays."""
    F = len(ids)
    out = dict(out_desc=np.zeros((F, 32), np.uint8), out_normal=np.zeros((F, 3), F32), out_dist=np.zeros((F, 2), F32),
               best_obs=np.full(F, -1, np.int32), best_median=np.zeros(F, np.int32), status=np.zeros(F, np.uint8))
    centres = [camera_centre(k["Tcw"]) for k in table] if what & REFRESH_NORMAL else None
    for f, pid in enumerate(ids):
        pid = int(pid)
        if not (points["flags"][pid] & 1):
            out["status"][f] = BAD
            continue
        obs = observations[pid]
        if not obs:
            out["status"][f] = NO_OBS
            continue
        st = 0
        if what & REFRESH_DESC:
            live = [(pos, table[k]["desc"][i]) for pos, (k, i) in enumerate(obs) if not table[k].get("bad")]
            if not live:
                st |= NO_LIVE_KF
            elif len(live) > OBS_MAX:
                st |= TOO_MANY
            else:
                best, med = select([d for _, d in live])
                out["out_desc"][f] = live[best][1]
                out["best_obs"][f], out["best_median"][f] = live[best][0], med
                st |= DESC_WRITTEN
        if what & REFRESH_NORMAL:
            ref = int(points["ref"][pid])
            idx = next((i for k, i in obs if k == ref), 0)             # observations[pRefKF]: map::operator[] of an absent key is 0
            level = int(table[ref]["kps_un"]["octave"][idx]) if idx < len(table[ref]["kps_un"]) else 0   # beyond n_kps: the padding
            if level < 0 or level >= prm["nlevels"]:
                st |= BAD_OCTAVE
            else:
                out["out_normal"][f], out["out_dist"][f] = normal_and_depth(prm, [centres[k] for k, _ in obs], centres[ref], level, points["xyz"][pid])
                st |= NORMAL_WRITTEN
        out["status"][f] = st
    return out


def covisibility(table, observations, pt_flags, kfs, th=15, ccap=None):
    """msl_covisibility.  table: keyframe dicts with held_id.  Returns dict(weight [items][n_tab], conn / conn_w [items][ccap], n_conn)."""
    n_tab, n_pts = len(table), len(observations)
    ccap = ccap or n_tab
    out = dict(weight=np.zeros((len(kfs), n_tab), np.int32), conn=np.full((len(kfs), ccap), -1, np.int32),
               conn_w=np.zeros((len(kfs), ccap), np.int32), n_conn=np.zeros(len(kfs), np.int32))
    for f, k in enumerate(kfs):
        w = out["weight"][f]
        for pid in table[k]["held_id"]:
            pid = int(pid)
            if pid < 0 or pid >= n_pts or not (pt_flags[pid] & 1):
                continue
            for kk, _ in observations[pid]:
                if kk != k:
                    w[kk] += 1
        if not w.any():
            continue
        pairs = [(int(w[j]), j) for j in range(n_tab) if w[j] > 0 and w[j] >= th]
        if not pairs:
            j = int(np.argmax(w))                                       # strict > in ascending order: the first maximum
            pairs = [(int(w[j]), j)]
        pairs.sort(reverse=True)                                        # sort ascending, then push_front
        out["n_conn"][f] = len(pairs)
        for r, (c, j) in enumerate(pairs[:ccap]):
            out["conn"][f, r], out["conn_w"][f, r] = j, c
    return out


# ---- the literal form on the object graph of tests/fuse_model.py ---------------------------------------------------------------------------
def is_bad(kf):
    return bool(getattr(kf, "bad", False))


def compute_distinctive_descriptors(mp):
    """src/MapPoint.cc:210-270.  Returns the position of the chosen observation in the map's iteration order (None: left unchanged)."""
    if mp.bad:
        return None
    observations = dict(mp.obs)
    if not observations:
        return None
    vDescriptors, pos = [], []
    for n, kid in enumerate(sorted(observations)):
        pKF = mp.g.kfs[kid]
        if not is_bad(pKF):
            vDescriptors.append(pKF.data["desc"][observations[kid]]); pos.append(n)
    if not vDescriptors:
        return None
    best, _ = select_descriptor(vDescriptors)
    mp.desc = vDescriptors[best].copy()
    return pos[best]


def update_normal_and_depth(mp, prm):
    """src/MapPoint.cc:282-322; mp.ref is mpRefKF's id.  Returns False when nothing is written."""
    if mp.bad:
        return False
    observations = dict(mp.obs)
    if not observations:
        return False
    pRefKF = mp.g.kfs[mp.ref]
    level = int(pRefKF.data["kps_un"]["octave"][observations.get(mp.ref, 0)])
    if level < 0 or level >= prm["nlevels"]:                            # pinned: undefined in the reference
        return False
    mp.normal, mp.dist = normal_and_depth(prm, [camera_centre(mp.g.kfs[kid].data["Tcw"]) for kid in sorted(observations)],
                                       camera_centre(pRefKF.data["Tcw"]), level, mp.xyz)
    return True


def update_connections(kf, th=15):
    """src/KeyFrame.cc:230-299 up to the ordered lists: None for the early return, else (KFcounter, mvpOrderedConnectedKeyFrames as ids,
    mvOrderedWeights)."""
    KFcounter = {}
    for pMP in kf.slots:
        if pMP is None:
            continue
        if pMP.bad:
            continue
        for kid in sorted(pMP.obs):
            if kid == kf.id:
                continue
            KFcounter[kid] = KFcounter.get(kid, 0) + 1
    if not KFcounter:
        return None
    nmax, pKFmax, vPairs = 0, None, []
    for kid in sorted(KFcounter):
        if KFcounter[kid] > nmax:
            nmax, pKFmax = KFcounter[kid], kid
        if KFcounter[kid] >= th:
            vPairs.append((KFcounter[kid], kid))
    if not vPairs:
        vPairs.append((nmax, pKFmax))
    vPairs.sort()
    lKFs, lWs = [], []
    for c, kid in vPairs:
        lKFs.insert(0, kid); lWs.insert(0, c)
    return KFcounter, lKFs, lWs


def graph_observations(g):
    """The CSR's content from a graph: per point id [(keyframe id, keypoint index)] in keyframe id order."""
    return [[(kid, mp.obs[kid]) for kid in sorted(mp.obs)] for mp in g.mps]


def graph_table(g):
    """g.table() with the bad flag of every keyframe."""
    return [dict(t, bad=is_bad(kf)) for t, kf in zip(g.table(), g.kfs)]


def graph_points(g):
    return dict(flags=np.array([0 if p.bad else 1 for p in g.mps], np.uint8), xyz=np.array([p.xyz for p in g.mps], F32).reshape(-1, 3),
                ref=np.array([p.ref for p in g.mps], np.int32))

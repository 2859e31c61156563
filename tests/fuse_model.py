"""A literal, sequential CPU model of the point half of LocalMapping::SearchInNeighbors (reference src/LocalMapping.cc:545-569):
ORBmatcher::Fuse (src/ORBmatcher.cc:408-546) with KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:469-504) and MapPoint::PredictScale
(src/MapPoint.cc:350-364), in three forms:

  fuse_map_points / fuse_candidates   what msl_fuse_map_points / msl_fuse_candidates compute: every item from the state on entry, the
                                      add / replace choice by the slot walk of include/msl.h
  search_in_neighbors_literal         the reference's statements in their order on a small object graph (MapPoint with its observation
                                      map, nObs, bad flag and descriptor; KeyFrame with its slots; AddObservation, Replace and
                                      ComputeDistinctiveDescriptors as src/MapPoint.cc:83-93, 154-187, 210-275)
  replay                              the caller's loop of INTEGRATION.md section 3m: the batched results consumed in order against the live
                                      objects, a survivor whose descriptor a Replace changed searched again

Test infrastructure only.  Float conventions as tests/local_match_model.py.  std::map<KeyFrame*, size_t> iterates in
pointer order in the reference; the model iterates in keyframe id order (the order only decides ties of ComputeDistinctiveDescriptors)."""
import math

import numpy as np

from tests import local_match_model as lm

F32 = np.float32
(NULL, BAD, IN_KEYFRAME, BEHIND, OUT_OF_IMAGE, DISTANCE, VIEW_ANGLE, NO_FEATURE, NO_CANDIDATE, ABOVE_TH_LOW, ADDED, REPLACED_BY_HELD, REPLACES_HELD,
 HELD_BAD, UNRESOLVED) = range(15)
CODES = ("NULL", "BAD", "IN_KEYFRAME", "BEHIND", "OUT_OF_IMAGE", "DISTANCE", "VIEW_ANGLE", "NO_FEATURE", "NO_CANDIDATE", "ABOVE_TH_LOW", "ADDED",
         "REPLACED_BY_HELD", "REPLACES_HELD", "HELD_BAD", "UNRESOLVED")
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(a, b):
    return int(_POP[np.bitwise_xor(a, b)].sum())


def params(fx, fy, cx, cy, bf, min_x, max_x, min_y, max_y, nlevels=8, scale_factor=1.2, th=3.0, th_low=50):
    """The camera, bounds and scale tables as the reference's ORBextractor / KeyFrame form them (float)."""
    sf = np.ones(nlevels, F32)
    for i in range(1, nlevels):
        sf[i] = sf[i - 1] * F32(scale_factor)
    return dict(fx=F32(fx), fy=F32(fy), cx=F32(cx), cy=F32(cy), bf=F32(bf), minX=F32(min_x), maxX=F32(max_x), minY=F32(min_y), maxY=F32(max_y),
                th=F32(th), nlevels=nlevels, scale_factors=sf, inv_level_sigma2=F32(1.0) / (sf * sf), log_scale_factor=F32(math.log(scale_factor)),
                th_low=int(th_low))


def grid_of(kf):
    """KeyFrame::mGrid from grid_cell: cell id (ix * 48 + iy) -> keypoint indices in insertion order."""
    g = {}
    for i, c in enumerate(kf["grid_cell"]):
        if c >= 0:
            g.setdefault(int(c), []).append(i)
    return g


def search_one(prm, kf, xyz, normal, dist, desc, margins=None, trace=None):
    """src/ORBmatcher.cc:433-525 for one map point against one keyframe.  Returns (status or None, bestIdx, bestDist): a status for an exit
    before or inside the search, None when the candidate loop ran and left a best distance below 256.  trace: dict filled with u, v, ur,
    level, n_indices (as msl_debug_fuse) and the events the coverage test counts."""
    m = margins if margins is not None else []
    tr = trace if trace is not None else {}
    tr.update(u=F32(0), v=F32(0), ur=F32(0), level=0, n_indices=0)
    fx, fy, cx, cy, bf = (F32(prm[k]) for k in ("fx", "fy", "cx", "cy", "bf"))
    minX, maxX, minY, maxY = (F32(prm[k]) for k in ("minX", "maxX", "minY", "maxY"))
    T = np.asarray(kf["Tcw"], F32).reshape(3, 4)
    tcw = T[:, 3]
    P = np.asarray(xyz, F32)
    Pc = lm.gemm3(T, False, 1.0, P, tcw)                               # :434
    m.append(("z", float(Pc[2]), 0.0, float(np.abs(Pc).max())))
    if Pc[2] < F32(0):                                                 # :437
        return BEHIND, -1, 256
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        invz = F32(1) / Pc[2]                                          # :440
        x = Pc[0] * invz; y = Pc[1] * invz
        u = fx * x + cx; v = fy * y + cy                               # :444
    tr["u"], tr["v"] = u, v
    w, h = float(maxX - minX), float(maxY - minY)
    m += [("minX", float(u), float(minX), w), ("maxX", float(u), float(maxX), w), ("minY", float(v), float(minY), h), ("maxY", float(v), float(maxY), h)]
    if not (u >= minX and u < maxX and v >= minY and v < maxY):        # KeyFrame::IsInImage, half-open
        return OUT_OF_IMAGE, -1, 256
    ur = u - bf * invz                                                 # :451
    tr["ur"] = ur
    maxDistance = F32(1.2) * F32(dist[1]); minDistance = F32(0.8) * F32(dist[0])
    Ow = lm.gemm3(T, True, -1.0, tcw)                                  # KeyFrame::SetPose
    PO = P - Ow
    dist3D = F32(math.sqrt(sum(float(PO[k]) * float(PO[k]) for k in range(3))))   # :456 cv::norm
    m += [("minDistance", float(dist3D), float(minDistance), float(minDistance)), ("maxDistance", float(dist3D), float(maxDistance), float(maxDistance))]
    if dist3D < minDistance or dist3D > maxDistance:                   # :459
        return DISTANCE, -1, 256
    Pn = np.asarray(normal, F32)
    dot = 0.0
    for k in range(3):
        dot += float(PO[k]) * float(Pn[k])
    m.append(("viewCos", dot, 0.5 * float(dist3D), float(dist3D)))
    if dot < 0.5 * float(dist3D):                                      # :465
        return VIEW_ANGLE, -1, 256
    nlevels = int(prm["nlevels"])
    level = lm.predict_scale(dist[1], dist3D, prm["log_scale_factor"], nlevels)   # :468
    q = float(F32(math.log(float(F32(dist[1]) / dist3D))) / F32(prm["log_scale_factor"]))
    if -0.5 < q < nlevels - 1.5:
        m.append(("ceil", q, float(round(q)), 1.0))
    tr["level"] = level
    radius = F32(prm["th"]) * prm["scale_factors"][level]              # :471
    kps = kf["kps_un"]
    un = np.stack([kps["x"], kps["y"]], 1) if len(kps) else np.zeros((0, 2), F32)
    idxs = lm.features_in_area(prm, kf.get("_grid") or grid_of(kf), kps, un, u, v, radius, -1, -1)   # :473, no level filter
    tr["n_indices"] = len(idxs)
    wInv = F32(lm.GRID_COLS) / (maxX - minX); hInv = F32(lm.GRID_ROWS) / (maxY - minY)
    tr["clipped_corner"] = bool(np.floor((u - minX - radius) * wInv) < 0 and np.floor((v - minY - radius) * hInv) < 0) or \
        bool(np.ceil((u - minX + radius) * wInv) > lm.GRID_COLS - 1 and np.ceil((v - minY + radius) * hInv) > lm.GRID_ROWS - 1)
    cx0, cx1 = max(0, int(np.floor((u - minX - radius) * wInv))), min(lm.GRID_COLS - 1, int(np.ceil((u - minX + radius) * wInv)))
    cy0, cy1 = max(0, int(np.floor((v - minY - radius) * hInv))), min(lm.GRID_ROWS - 1, int(np.ceil((v - minY + radius) * hInv)))
    tr["cells"] = max(0, cx1 - cx0 + 1) * max(0, cy1 - cy0 + 1)        # the window's cells
    if not idxs:                                                       # :475
        return NO_FEATURE, -1, 256
    bestDist, bestIdx = 256, -1
    chi = tr.setdefault("chi", set()); ties = tr.setdefault("ties", [])
    for idx in idxs:
        kpLevel = int(kps["octave"][idx])
        if kpLevel < level - 1 or kpLevel > level:                     # :491
            continue
        if kpLevel < 0 or kpLevel >= nlevels:                          # pinned: not an octave of this pyramid
            continue
        kpx, kpy, kpr = F32(kps["x"][idx]), F32(kps["y"][idx]), F32(kf["uright"][idx])
        ex = u - kpx; ey = v - kpy
        inv = F32(prm["inv_level_sigma2"][kpLevel])
        if kpr >= F32(0):                                              # :494
            er = ur - kpr
            e2 = ex * ex + ey * ey + er * er
            m.append(("chi3", float(e2 * inv), 7.8, 7.8))
            bad = float(e2 * inv) > 7.8
            chi.add(("stereo", not bad))
        else:
            e2 = ex * ex + ey * ey
            m.append(("chi2", float(e2 * inv), 5.99, 5.99))
            bad = float(e2 * inv) > 5.99
            chi.add(("mono", not bad))
        if bad:
            continue
        d = hamming(np.asarray(desc, np.uint8), kf["desc"][idx])
        if d == bestDist and bestIdx >= 0:
            ties.append((bestIdx, idx, int(kf["grid_cell"][bestIdx]), int(kf["grid_cell"][idx])))
        if d < bestDist:                                               # :521
            bestDist, bestIdx = d, idx
    if bestIdx < 0:
        return NO_CANDIDATE, -1, 256
    return None, bestIdx, bestDist


def fuse_item(prm, kf, points, lst, margins=None):
    """One item of msl_fuse_map_points: Fuse(kf, lst) from the state on entry with the slot walk of include/msl.h."""
    n = len(lst)
    out = dict(best_idx=np.full(n, -1, np.int32), best_dist=np.full(n, 256, np.int32), status=np.zeros(n, np.uint8), other=np.full(n, -1, np.int32),
               n_fused=0, trace=[None] * n, equal_nobs=0)
    flags, nobs = points["flags"], points["nobs"]
    n_pts = len(flags)
    held = [int(h) if 0 <= int(h) < n_pts else -1 for h in kf["held_id"]]
    in_kf = set(h for h in held if h >= 0)
    kf = dict(kf, _grid=grid_of(kf))
    slot = {}                                                          # s -> [holder, bad, nobs, stale]
    for j, p in enumerate(lst):
        p = int(p)
        tr = out["trace"][j] = dict(u=F32(0), v=F32(0), ur=F32(0), level=0, n_indices=0)
        if p < 0:                                                      # :427
            out["status"][j] = NULL
            continue
        if not (flags[p] & 1):                                         # :430
            out["status"][j] = BAD
            continue
        if p in in_kf:
            out["status"][j] = IN_KEYFRAME
            continue
        st, bi, bd = search_one(prm, kf, points["xyz"][p], points["normal"][p], points["dist"][p], points["desc"][p], margins, tr)
        if st is not None:
            out["status"][j] = st
            continue
        out["best_idx"][j], out["best_dist"][j] = bi, bd
        if bd > int(prm["th_low"]):                                    # :528
            out["status"][j] = ABOVE_TH_LOW
            continue
        out["n_fused"] += 1
        if bi not in slot:
            h = held[bi]
            slot[bi] = [h, h >= 0 and not (flags[h] & 1), int(nobs[h]) if h >= 0 else 0, False]
        s = slot[bi]
        out["other"][j] = s[0]
        if s[0] < 0:
            out["status"][j] = ADDED
            slot[bi] = [p, False, int(nobs[p]) + (2 if kf["uright"][bi] >= 0 else 1), False]
        elif s[1]:
            out["status"][j] = HELD_BAD
        elif s[3]:
            out["status"][j] = UNRESOLVED
        elif s[2] > int(nobs[p]):
            out["status"][j] = REPLACED_BY_HELD
            s[3] = True
        else:
            out["equal_nobs"] += int(s[2] == int(nobs[p]))
            out["status"][j] = REPLACES_HELD
            s[0] = p; s[3] = True
    return out


def fuse_map_points(prm, table, points, items, lists, margins=None):
    """msl_fuse_map_points: items [(target table index, list index)] -> one fuse_item result per item."""
    return [fuse_item(prm, table[t], points, lists[l], margins) for t, l in items]


def fuse_candidates(table, points, items, lcap=None):
    """msl_fuse_candidates: items [[target table index, ...]] -> per item (the ids kept, at most lcap of them; the full count)."""
    res = []
    n_pts = len(points["flags"])
    for targets in items:
        seen, lst = set(), []
        for t in targets:
            for h in table[t]["held_id"]:
                h = int(h)
                if h < 0 or h >= n_pts:
                    continue
                if not (points["flags"][h] & 1) or h in seen:         # :562
                    continue
                seen.add(h); lst.append(h)
        res.append((lst if lcap is None else lst[:lcap], len(lst)))
    return res


# ---- the object graph -----------------------------------------------------------------------------------------------------------------------
class MapPoint:
    def __init__(self, g, mid, xyz, normal, dist):
        self.g, self.id, self.xyz, self.normal, self.dist = g, mid, np.asarray(xyz, F32), np.asarray(normal, F32), np.asarray(dist, F32)
        self.obs, self.nobs, self.bad, self.replaced, self.desc = {}, 0, False, None, np.zeros(32, np.uint8)

    def add_observation(self, kf, idx):                                # src/MapPoint.cc:83-93
        if kf.id in self.obs:
            return
        self.obs[kf.id] = idx
        self.nobs += 2 if kf.data["uright"][idx] >= 0 else 1

    def is_in_keyframe(self, kf):
        return kf.id in self.obs

    def replace(self, other):                                          # :154-187
        if other.id == self.id:
            return
        obs, self.obs, self.bad, self.replaced = self.obs, {}, True, other
        for kid in sorted(obs):
            kf = self.g.kfs[kid]
            if not other.is_in_keyframe(kf):
                kf.slots[obs[kid]] = other                             # ReplaceMapPointMatch
                other.add_observation(kf, obs[kid])
            else:
                kf.slots[obs[kid]] = None                              # EraseMapPointMatch
        other.compute_distinctive_descriptors()

    def compute_distinctive_descriptors(self):                         # :210-275
        if self.bad or not self.obs:
            return
        descs = [self.g.kfs[kid].data["desc"][self.obs[kid]] for kid in sorted(self.obs)]
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
        self.desc = descs[best].copy()


class KeyFrame:
    def __init__(self, kid, data):
        self.id, self.data, self.slots = kid, data, [None] * len(data["kps_un"])


class Graph:
    """Keyframes (id = table index) and map points (id = point table index)."""

    def __init__(self, kf_data):
        self.kfs = [KeyFrame(k, d) for k, d in enumerate(kf_data)]
        self.mps = []

    def new_point(self, xyz, normal, dist):
        self.mps.append(MapPoint(self, len(self.mps), xyz, normal, dist))
        return self.mps[-1]

    def observe(self, mp, kid, idx):
        kf = self.kfs[kid]
        mp.add_observation(kf, idx); kf.slots[idx] = mp

    def table(self):
        return [dict(kf.data, held_id=np.array([-1 if s is None else s.id for s in kf.slots], np.int32)) for kf in self.kfs]

    def points(self):
        m = self.mps
        return dict(xyz=np.array([p.xyz for p in m], F32).reshape(-1, 3), normal=np.array([p.normal for p in m], F32).reshape(-1, 3),
                    dist=np.array([p.dist for p in m], F32).reshape(-1, 2), desc=np.array([p.desc for p in m], np.uint8).reshape(-1, 32),
                    flags=np.array([0 if p.bad else 1 for p in m], np.uint8), nobs=np.array([p.nobs for p in m], np.int32))

    def snapshot(self):
        """Everything the two ways of running SearchInNeighbors must leave equal."""
        return dict(slots=[[-1 if s is None else s.id for s in kf.slots] for kf in self.kfs],
                    points=[(dict(p.obs), p.nobs, p.bad, p.desc.tobytes(), None if p.replaced is None else p.replaced.id) for p in self.mps])


def _fuse_literal(prm, kf, vpMapPoints):
    """ORBmatcher::Fuse, statement by statement, on live objects."""
    nFused = 0
    for pMP in vpMapPoints:
        if pMP is None:
            continue
        if pMP.bad or pMP.is_in_keyframe(kf):
            continue
        st, bestIdx, bestDist = search_one(prm, kf.data, pMP.xyz, pMP.normal, pMP.dist, pMP.desc)
        if st is not None:
            continue
        if bestDist <= int(prm["th_low"]):
            pMPinKF = kf.slots[bestIdx]
            if pMPinKF is not None:
                if not pMPinKF.bad:
                    if pMPinKF.nobs > pMP.nobs:
                        pMP.replace(pMPinKF)
                    else:
                        pMPinKF.replace(pMP)
            else:
                pMP.add_observation(kf, bestIdx)
                kf.slots[bestIdx] = pMP
            nFused += 1
    return nFused


def search_in_neighbors_literal(g, prm, cur, targets):
    """src/LocalMapping.cc:545-569 on the graph g: returns the return value of every Fuse call, the last one's into the current keyframe."""
    pCur = g.kfs[cur]
    vpMapPointMatches = list(pCur.slots)
    rets = [_fuse_literal(prm, g.kfs[t], vpMapPointMatches) for t in targets]
    vpFuseCandidates, marked = [], set()
    for t in targets:
        for pMP in list(g.kfs[t].slots):
            if pMP is None:
                continue
            if pMP.bad or pMP.id in marked:
                continue
            marked.add(pMP.id)
            vpFuseCandidates.append(pMP)
    rets.append(_fuse_literal(prm, pCur, vpFuseCandidates))
    return rets


class ModelEntry:
    """The two batched entries as the replay calls them; tests/test_fuse_gpu.py substitutes the device's."""

    def __init__(self):
        self.calls = []                                                # (table, points, items, lists, results) of every fuse call

    def candidates(self, table, points, items):
        return [lst for lst, _ in fuse_candidates(table, points, items)]

    def fuse(self, prm, table, points, items, lists):
        res = fuse_map_points(prm, table, points, items, lists)
        self.calls.append((table, points, items, lists, res))
        return res


def _replay_item(g, prm, entry, kf, lst, res, first, stats):
    """One Fuse call replayed: res is the item's batched result (state on entry: when the item began if `first`, else earlier)."""
    entry_desc = res["_desc"]
    nFused = 0
    for j, p in enumerate(lst):
        if p < 0:
            continue
        pMP = g.mps[p]
        if pMP.bad or pMP.is_in_keyframe(kf):                          # live; the skip is monotone
            continue
        assert res["status"][j] not in (NULL, BAD, IN_KEYFRAME)
        bi, bd, st = int(res["best_idx"][j]), int(res["best_dist"][j]), int(res["status"][j])
        if pMP.desc.tobytes() != entry_desc[p].tobytes():              # a Replace gave the survivor a new descriptor: search it again
            one = entry.fuse(prm, g.table(), g.points(), [(kf.id, 0)], [[p]])[0]
            bi, bd, st = int(one["best_idx"][0]), int(one["best_dist"][0]), -1
            stats["researched"] += 1
            stats["research_changed"] += int((bi, bd) != (int(res["best_idx"][j]), int(res["best_dist"][j])))
        if bd > int(prm["th_low"]) or bi < 0:
            continue
        pMPinKF = kf.slots[bi]
        if pMPinKF is not None:
            if not pMPinKF.bad:
                if pMPinKF.nobs > pMP.nobs:
                    did = REPLACED_BY_HELD
                    pMP.replace(pMPinKF)
                else:
                    did = REPLACES_HELD
                    pMPinKF.replace(pMP)
                stats[CODES[did]] += 1
            else:
                did = HELD_BAD
        else:
            did = ADDED
            pMP.add_observation(kf, bi)
            kf.slots[bi] = pMP
        if first and st >= 0 and st != UNRESOLVED:                     # the item's entry state was the live state: the device's choice is the live one
            assert st == did, (j, p, CODES[st], CODES[did])
        nFused += 1
    return nFused


def replay(g, prm, cur, targets, entry=None):
    """The caller's SearchInNeighbors on the batched entries: two msl_fuse_map_points calls (the targets sharing one list, then the
    current keyframe with msl_fuse_candidates' list), each replayed in order against the live objects.  Returns (rets, stats)."""
    entry = entry or ModelEntry()
    stats = dict(REPLACED_BY_HELD=0, REPLACES_HELD=0, researched=0, research_changed=0, UNRESOLVED=0)
    pCur = g.kfs[cur]
    rets = []
    lst = [-1 if s is None else s.id for s in pCur.slots]
    seen = set()
    lst = [(-1 if (p in seen or seen.add(p)) else p) if p >= 0 else -1 for p in lst]      # later duplicates are NULLed (exact, msl.h)
    points = g.points()
    if targets:
        res = entry.fuse(prm, g.table(), points, [(t, 0) for t in targets], [lst])
        for i, t in enumerate(targets):
            res[i]["_desc"] = points["desc"]
            stats["UNRESOLVED"] += int((np.asarray(res[i]["status"]) == UNRESOLVED).sum())
            rets.append(_replay_item(g, prm, entry, g.kfs[t], lst, res[i], i == 0, stats))
    table, points = g.table(), g.points()
    cand = entry.candidates(table, points, [list(targets)])[0]
    res = entry.fuse(prm, table, points, [(cur, 0)], [cand])[0]
    res["_desc"] = points["desc"]
    stats["UNRESOLVED"] += int((np.asarray(res["status"]) == UNRESOLVED).sum())
    rets.append(_replay_item(g, prm, entry, pCur, cand, res, True, stats))
    return rets, stats

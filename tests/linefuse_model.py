"""A literal, sequential CPU model of the line half of LocalMapping::SearchInNeighbors (reference src/LocalMapping.cc:583-618):
LSDmatcher::Fuse (src/LSDmatcher.cpp:259-382) with KeyFrame::GetLinesInArea (src/KeyFrame.cc:506-538), MapLine::PredictScale
(src/MapLine.cpp:320-328) and MapLine::UpdateAverageDir (:262-308), in three forms:

  fuse_map_lines / update_average_dir   what msl_fuse_map_lines / msl_refresh_map_lines compute: every item from the state on entry, the
                                        add / replace choice by the slot walk of include/msl.h
  search_in_neighbors_lines_literal     the reference's statements in their order on a small object graph (MapLine with its observation map,
                                        nObs, bad flag and descriptor; KeyFrame with its slots; AddObservation, Replace and
                                        ComputeDistinctiveDescriptors as src/MapLine.cpp:75-83, 139-172, 195-255), fuse_literal being one
                                        LSDmatcher::Fuse call
  replay                                the caller's loop of INTEGRATION.md section 3o: the batched results consumed in order against the live
                                        objects; no IsInKeyFrame skip, the self-hit counted, a survivor whose descriptor a Replace changed
                                        searched again

Test infrastructure only.  Float conventions as tests/line_match_model.py.  std::map<KeyFrame*, size_t> iterates in
pointer order in the reference; the model iterates in keyframe id order."""
import math

import numpy as np

from tests.fuse_model import fuse_candidates, hamming
from tests.line_match_model import clamp_level, get_lines_in_area, predict_level, wrap
from tests.line_match_model import project_line as _project_line
from tests.local_match_model import gemm3

F32 = np.float32
INT_MAX = 2 ** 31 - 1
(NULL, BAD, BEHIND, OUT_OF_IMAGE, DISTANCE, VIEW_ANGLE, NO_FEATURE, NO_CANDIDATE, ABOVE_TH_LOW, ADDED, REPLACED_BY_HELD, REPLACES_HELD, HELD_BAD,
 UNRESOLVED, SELF) = range(15)
CODES = ("NULL", "BAD", "BEHIND", "OUT_OF_IMAGE", "DISTANCE", "VIEW_ANGLE", "NO_FEATURE", "NO_CANDIDATE", "ABOVE_TH_LOW", "ADDED", "REPLACED_BY_HELD",
         "REPLACES_HELD", "HELD_BAD", "UNRESOLVED", "SELF")
NORMAL_WRITTEN, R_BAD, NO_OBS, BAD_OCTAVE = 2, 4, 8, 64                  # the MSL_REFRESH_* bits msl_refresh_map_lines uses


def params(fx, fy, cx, cy, min_x, max_x, min_y, max_y, nlevels=8, scale_factor=1.2, th=3.0, th_low=50):
    """The camera, bounds and scale table as the reference's KeyFrame holds them (float)."""
    sf = np.ones(nlevels, F32)
    for i in range(1, nlevels):
        sf[i] = sf[i - 1] * F32(scale_factor)
    return dict(fx=F32(fx), fy=F32(fy), cx=F32(cx), cy=F32(cy), minX=F32(min_x), maxX=F32(max_x), minY=F32(min_y), maxY=F32(max_y), th=F32(th),
                nlevels=nlevels, scale_factors=sf, log_scale_factor=F32(math.log(scale_factor)), th_low=int(th_low))


def _finite(*v):
    return all(math.isfinite(float(x)) for x in v)


def search_one(prm, kf, xyz, normal, dist, desc, margins=None, trace=None):
    """src/LSDmatcher.cpp:283-362 for one map line against one keyframe.  Returns (status or None, bestIdx, bestDist): a status for an
    exit before or inside the search, None when a keyline passed the level window.  trace: dict filled with u1, v1, u2, v2, radius, level,
    n_indices (as msl_debug_line_fuse)."""
    m = margins if margins is not None else []
    tr = trace if trace is not None else {}
    tr.update(u1=F32(0), v1=F32(0), u2=F32(0), v2=F32(0), radius=F32(0), level=0, n_indices=0)
    T = np.asarray(kf["Tcw"], F32).reshape(3, 4)
    res = _project_line(prm, T, xyz)                                   # :283-317
    SPc = gemm3(T, False, 1.0, np.asarray(xyz, np.float64)[:3].astype(F32), T[:, 3])
    EPc = gemm3(T, False, 1.0, np.asarray(xyz, np.float64)[3:6].astype(F32), T[:, 3])
    if SPc[2] != 0 and EPc[2] != 0:
        m += [("z1", float(SPc[2]), 0.0, float(np.abs(SPc).max())), ("z2", float(EPc[2]), 0.0, float(np.abs(EPc).max()))]
    if res is None:
        if SPc[2] < F32(0) or EPc[2] < F32(0):
            return BEHIND, -1, INT_MAX
        return OUT_OF_IMAGE, -1, INT_MAX
    u1, v1, u2, v2, SP, EP = res
    tr.update(u1=u1, v1=v1, u2=u2, v2=v2)
    w, h = float(prm["maxX"] - prm["minX"]), float(prm["maxY"] - prm["minY"])
    if _finite(u1, v1, u2, v2):
        for u, v in ((u1, v1), (u2, v2)):
            m += [("minX", float(u), float(prm["minX"]), w), ("maxX", float(u), float(prm["maxX"]), w), ("minY", float(v), float(prm["minY"]), h),
                  ("maxY", float(v), float(prm["maxY"]), h)]
    maxDistance = F32(1.2) * F32(dist[1]); minDistance = F32(0.8) * F32(dist[0])   # :319-320
    Ow = gemm3(T, True, -1.0, T[:, 3])                                 # KeyFrame::SetPose
    with np.errstate(over="ignore", invalid="ignore"):
        OM = (SP * F32(0.5) + EP * F32(0.5) + F32(0)) - Ow             # :322, the addWeighted pin of tests/line_match_model.py
    s = 0.0
    for k in range(3):
        s += float(OM[k]) * float(OM[k])
    d = F32(math.sqrt(s)) if s == s else F32(np.nan)                   # :323 cv::norm
    if _finite(d):
        m += [("minDistance", float(d), float(minDistance), float(minDistance)), ("maxDistance", float(d), float(maxDistance), float(maxDistance))]
    if d < minDistance or d > maxDistance:                             # :325 (a NaN passes)
        return DISTANCE, -1, INT_MAX
    pn = np.asarray(normal, np.float64).astype(F32)                    # :329
    dot = 0.0
    for k in range(3):
        dot += float(OM[k]) * float(pn[k])
    if _finite(d, dot):
        m.append(("viewCos", dot, 0.5 * float(d), float(d)))
    if dot < 0.5 * float(d):                                           # :331
        return VIEW_ANGLE, -1, INT_MAX
    nlevels = int(prm["nlevels"])
    L = predict_level(dist[1], d, prm["log_scale_factor"])             # :334, not clamped
    if _finite(d) and float(d) > 0 and float(dist[1]) > 0:
        q = float(F32(math.log(float(F32(dist[1]) / d))) / F32(prm["log_scale_factor"]))
        m.append(("ceil", q, float(round(q)), 1.0))
    radius = F32(prm["th"]) * F32(prm["scale_factors"][clamp_level(L, nlevels)])   # :336, the index clamped for the lookup only
    tr.update(radius=radius, level=L)
    kl = kf["kl"]
    idxs = get_lines_in_area(kl, u1, v1, u2, v2, radius)               # :338, levels -1 / -1
    tr["n_indices"] = len(idxs)
    if _finite(u1, v1, u2, v2) and u1 != u2:
        mx, my = 0.5 * float(u1 + u2), 0.5 * float(v1 + v2)
        rr, rs = float(radius * radius), float(radius) * 0.01
        slope0 = (v1 - v2) / (u1 - u2)
        for i in range(len(kl)):
            dd = float(F32((mx - float(kl["x"][i])) ** 2 + (my - float(kl["y"][i])) ** 2))
            m.append(("area", dd, rr, rr))
            if dd <= rr:
                m.append(("slope", float(slope0 - F32(kl["angle"][i])), rs, rs))
    if not idxs:                                                       # :340
        return NO_FEATURE, -1, INT_MAX
    bestDist, bestIdx = INT_MAX, -1
    for idx in idxs:
        klLevel = int(kl["octave"][idx])
        if klLevel < wrap(L - 1) or klLevel > L:                       # :351
            continue
        dd = hamming(np.asarray(desc, np.uint8), kf["ldesc"][idx])
        if dd < bestDist:                                              # :358
            bestDist, bestIdx = dd, idx
    if bestIdx < 0:
        return NO_CANDIDATE, -1, INT_MAX
    return None, bestIdx, bestDist


def fuse_item(prm, kf, lines, lst, margins=None):
    """One item of msl_fuse_map_lines: Fuse(kf, lst) from the state on entry with the slot walk of include/msl.h."""
    n = len(lst)
    out = dict(best_idx=np.full(n, -1, np.int32), best_dist=np.full(n, INT_MAX, np.int32), status=np.zeros(n, np.uint8),
               other=np.full(n, -1, np.int32), n_fused=0, trace=[None] * n, added_in_kf=0)
    flags, nobs = lines["flags"], lines["nobs"]
    n_lines = len(flags)
    held = [int(h) if 0 <= int(h) < n_lines else -1 for h in kf["held_id"]]
    in_kf = set(h for h in held if h >= 0)
    slot = {}                                                          # s -> [holder, bad, nobs, stale]
    for j, p in enumerate(lst):
        p = int(p)
        tr = out["trace"][j] = dict(u1=F32(0), v1=F32(0), u2=F32(0), v2=F32(0), radius=F32(0), level=0, n_indices=0)
        if p < 0:                                                      # :280
            out["status"][j] = NULL
            continue
        if not (flags[p] & 1):
            out["status"][j] = BAD
            continue
        st, bi, bd = search_one(prm, kf, lines["xyz"][p], lines["normal"][p], lines["dist"][p], lines["desc"][p], margins, tr)
        if st is not None:
            out["status"][j] = st
            continue
        out["best_idx"][j], out["best_dist"][j] = bi, bd
        if bd > int(prm["th_low"]):                                    # :364
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
            out["added_in_kf"] += int(p in in_kf)
            slot[bi] = [p, False, int(nobs[p]) + (0 if p in in_kf else 1), False]   # src/MapLine.cpp:77: no new observation
        elif s[1]:
            out["status"][j] = HELD_BAD
        elif s[3]:
            out["status"][j] = UNRESOLVED
        elif s[0] == p:
            out["status"][j] = SELF                                    # src/MapLine.cpp:140
        elif s[2] > int(nobs[p]):
            out["status"][j] = REPLACED_BY_HELD
            s[3] = True
        else:
            out["status"][j] = REPLACES_HELD
            s[0] = p; s[3] = True
    return out


def fuse_map_lines(prm, table, lines, items, lists, margins=None):
    """msl_fuse_map_lines: items [(target table index, list index)] -> one fuse_item result per item."""
    return [fuse_item(prm, table[t], lines, lists[l], margins) for t, l in items]


def update_average_dir(prm, table, xyz6, obs, ref, bad=False):
    """msl_refresh_map_lines for one line (src/MapLine.cpp:262-308): obs = [(keyframe table index, keyline index), ...] in the map's order,
    ref = the table index of mpRefKF.  Returns (status, normal (3,) f64, dist (2,) f32); zeros where nothing is written."""
    zero = (np.zeros(3, np.float64), np.zeros(2, F32))
    if bad:                                                            # :269
        return (R_BAD,) + zero
    if not obs:                                                        # :276
        return (NO_OBS,) + zero
    P = np.asarray(xyz6, np.float64)
    normal = np.zeros(3, np.float64)
    n = 0
    ref_idx = 0                                                        # observations[pRefKF] of an absent key
    seen_ref = False
    for k, idx in obs:
        T = np.asarray(table[k]["Tcw"], F32).reshape(3, 4)
        OWi = gemm3(T, True, -1.0, T[:, 3]).astype(np.float64)         # :284-285
        middle = 0.5 * (P[:3] + P[3:6])                                # :286
        ni = middle - OWi
        with np.errstate(divide="ignore", invalid="ignore"):
            norm = math.sqrt(ni[0] * ni[0] + (ni[1] * ni[1] + ni[2] * ni[2]))   # Eigen's unrolled 3-vector reduction
            normal = normal + ni / np.float64(norm)                    # :288
        n += 1
        if k == ref and not seen_ref:
            ref_idx, seen_ref = idx, True
    nlevels = int(prm["nlevels"])
    if not (0 <= ref < len(table)) or not (0 <= ref_idx < len(table[ref]["kl"])):
        return (BAD_OCTAVE,) + zero
    level = int(table[ref]["kl"]["octave"][ref_idx])                   # :298
    if level < 0 or level >= nlevels:
        return (BAD_OCTAVE,) + zero
    T = np.asarray(table[ref]["Tcw"], F32).reshape(3, 4)
    SP, EP = P[:3].astype(F32), P[3:6].astype(F32)
    CM = (SP * F32(0.5) + EP * F32(0.5) + F32(0)) - gemm3(T, True, -1.0, T[:, 3])   # :292-296
    s = 0.0
    for k in range(3):
        s += float(CM[k]) * float(CM[k])
    d = F32(math.sqrt(s))                                              # :297
    dmax = d * F32(prm["scale_factors"][level])                        # :304
    dmin = dmax / F32(prm["scale_factors"][nlevels - 1])               # :305
    return NORMAL_WRITTEN, normal / np.float64(n), np.array([dmin, dmax], F32)


# ---- the object graph -----------------------------------------------------------------------------------------------------------------------
class MapLine:
    def __init__(self, g, mid, xyz, normal, dist, ref):
        self.g, self.id, self.xyz, self.normal, self.dist, self.ref = g, mid, np.asarray(xyz, np.float64), np.asarray(normal, np.float64), np.asarray(dist, F32), ref
        self.obs, self.nobs, self.bad, self.replaced, self.desc = {}, 0, False, None, np.zeros(32, np.uint8)

    def add_observation(self, kf, idx):                                # src/MapLine.cpp:75-83
        if kf.id in self.obs:
            return
        self.obs[kf.id] = idx
        self.nobs += 1

    def is_in_keyframe(self, kf):
        return kf.id in self.obs

    def replace(self, other):                                          # :139-172
        if other.id == self.id:
            return
        obs, self.obs, self.bad, self.replaced = self.obs, {}, True, other
        for kid in sorted(obs):
            kf = self.g.kfs[kid]
            if not other.is_in_keyframe(kf):
                kf.slots[obs[kid]] = other                             # ReplaceMapLineMatch
                other.add_observation(kf, obs[kid])
            else:
                kf.slots[obs[kid]] = None                              # EraseMapLineMatch
        other.compute_distinctive_descriptors()

    def observations(self):
        """The observation list in the map's order: [(keyframe id, keyline index), ...]."""
        return [(kid, self.obs[kid]) for kid in sorted(self.obs)]

    def compute_distinctive_descriptors(self):                         # :195-255
        if self.bad or not self.obs:
            return
        descs = [self.g.kfs[kid].data["ldesc"][self.obs[kid]] for kid in sorted(self.obs)]
        N = len(descs)
        D = np.zeros((N, N), np.int64)
        for i in range(N):
            for j in range(N):
                D[i, j] = hamming(descs[i], descs[j])
        best_median, best = INT_MAX, 0
        for i in range(N):
            median = int(np.sort(D[i])[int(0.5 * (N - 1))])
            if median < best_median:
                best_median, best = median, i
        self.desc = descs[best].copy()

    def update_average_dir(self, prm):                                 # :262-308
        st, normal, dist = update_average_dir(prm, [kf.data for kf in self.g.kfs], self.xyz, self.observations(), self.ref, self.bad)
        if st == NORMAL_WRITTEN:
            self.normal, self.dist = normal, dist
        return st


class KeyFrame:
    def __init__(self, kid, data):
        self.id, self.data, self.slots = kid, data, [None] * len(data["kl"])


class Graph:
    """Keyframes (id = table index) and map lines (id = line table index)."""

    def __init__(self, kf_data):
        self.kfs = [KeyFrame(k, d) for k, d in enumerate(kf_data)]
        self.mls = []

    def new_line(self, xyz, normal, dist, ref):
        self.mls.append(MapLine(self, len(self.mls), xyz, normal, dist, ref))
        return self.mls[-1]

    def observe(self, ml, kid, idx):
        kf = self.kfs[kid]
        ml.add_observation(kf, idx); kf.slots[idx] = ml

    def table(self):
        return [dict(kf.data, held_id=np.array([-1 if s is None else s.id for s in kf.slots], np.int32)) for kf in self.kfs]

    def lines(self):
        m = self.mls
        return dict(xyz=np.array([p.xyz for p in m], np.float64).reshape(-1, 6), normal=np.array([p.normal for p in m], np.float64).reshape(-1, 3),
                    dist=np.array([p.dist for p in m], F32).reshape(-1, 2), desc=np.array([p.desc for p in m], np.uint8).reshape(-1, 32),
                    flags=np.array([0 if p.bad else 1 for p in m], np.uint8), nobs=np.array([p.nobs for p in m], np.int32),
                    ref=np.array([p.ref for p in m], np.int32))

    def snapshot(self):
        """Everything the two ways of running SearchInNeighbors must leave equal."""
        return dict(slots=[[-1 if s is None else s.id for s in kf.slots] for kf in self.kfs],
                    lines=[(dict(p.obs), p.nobs, p.bad, p.desc.tobytes(), None if p.replaced is None else p.replaced.id, p.normal.tobytes(),
                            p.dist.tobytes()) for p in self.mls])


def fuse_literal(prm, kf, vpMapLines):
    """LSDmatcher::Fuse, statement by statement, on live objects."""
    nFused = 0
    for pML in vpMapLines:
        if pML is None or pML.bad:                                     # :280
            continue
        st, bestIdx, bestDist = search_one(prm, kf.data, pML.xyz, pML.normal, pML.dist, pML.desc)
        if st is not None:
            continue
        if bestDist <= int(prm["th_low"]):                             # :364
            pMLinKF = kf.slots[bestIdx]
            if pMLinKF is not None:
                if not pMLinKF.bad:
                    if pMLinKF.nobs > pML.nobs:
                        pML.replace(pMLinKF)
                    else:
                        pMLinKF.replace(pML)
            else:
                pML.add_observation(kf, bestIdx)
                kf.slots[bestIdx] = pML
            nFused += 1
    return nFused


def line_candidates_literal(g, targets):
    """vpLineFuseCandidates, src/LocalMapping.cc:589-605."""
    out, marked = [], set()
    for t in targets:
        for pML in list(g.kfs[t].slots):
            if pML is None:
                continue
            if pML.bad or pML.id in marked:
                continue
            marked.add(pML.id)
            out.append(pML)
    return out


def refresh_literal(g, prm, cur):
    """src/LocalMapping.cc:609-618."""
    for pML in list(g.kfs[cur].slots):
        if pML is not None and not pML.bad:
            pML.compute_distinctive_descriptors()
            pML.update_average_dir(prm)


def search_in_neighbors_lines_literal(g, prm, cur, targets):
    """src/LocalMapping.cc:583-618 on the graph g: returns the return value of every Fuse call, the last one's into the current keyframe."""
    pCur = g.kfs[cur]
    vpMapLineMatches = list(pCur.slots)
    rets = [fuse_literal(prm, g.kfs[t], vpMapLineMatches) for t in targets]
    rets.append(fuse_literal(prm, pCur, line_candidates_literal(g, targets)))
    refresh_literal(g, prm, cur)
    return rets


class ModelEntry:
    """The batched entries as the replay calls them; tests/test_linefuse_gpu.py substitutes the device's."""

    def __init__(self):
        self.calls = []                                                # (table, lines, items, lists, results) of every fuse call

    def candidates(self, table, lines, items):
        return [lst for lst, _ in fuse_candidates(table, lines, items)]

    def fuse(self, prm, table, lines, items, lists):
        res = fuse_map_lines(prm, table, lines, items, lists)
        self.calls.append((table, lines, items, lists, res))
        return res

    def refresh(self, g, prm, ids):
        """ComputeDistinctiveDescriptors and UpdateAverageDir of the live lines ids, written into the objects."""
        for i in ids:
            g.mls[i].compute_distinctive_descriptors()
            g.mls[i].update_average_dir(prm)


def _replay_item(g, prm, entry, kf, orig, res, first, stats):
    """One Fuse call replayed: orig is the reference's own list (duplicates included), res the batched result of the list with later
    duplicates NULLed (state on entry: when the item began if `first`, else earlier)."""
    entry_desc = res["_desc"]
    nFused = 0
    first_j, dirty = {}, set()
    for j, p in enumerate(orig):
        if p < 0:
            continue
        jj = first_j.setdefault(p, j)                                  # a repeated line: the search of its first occurrence
        stats["repeated"] += int(jj != j)
        pML = g.mls[p]
        if pML.bad:                                                    # live; no IsInKeyFrame skip
            continue
        assert res["status"][jj] not in (NULL, BAD)
        bi, bd, st = int(res["best_idx"][jj]), int(res["best_dist"][jj]), int(res["status"][jj])
        if pML.desc.tobytes() != entry_desc[p].tobytes():              # a Replace gave the survivor a new descriptor: search it again
            one = entry.fuse(prm, g.table(), g.lines(), [(kf.id, 0)], [[p]])[0]
            bi, bd, st = int(one["best_idx"][0]), int(one["best_dist"][0]), -1
            stats["researched"] += 1
            stats["research_changed"] += int((bi, bd) != (int(res["best_idx"][jj]), int(res["best_dist"][jj])))
        if bd > int(prm["th_low"]) or bi < 0:
            continue
        pMLinKF = kf.slots[bi]
        clean = p not in dirty and (pMLinKF is None or pMLinKF.id not in dirty)
        if pMLinKF is not None:
            if not pMLinKF.bad:
                if pMLinKF is pML:
                    did = SELF                                         # Replace returns at once
                elif pMLinKF.nobs > pML.nobs:
                    did = REPLACED_BY_HELD
                    pML.replace(pMLinKF)
                else:
                    did = REPLACES_HELD
                    pMLinKF.replace(pML)
                if did != SELF:
                    dirty |= {p, pMLinKF.id}
                stats[CODES[did]] += 1
            else:
                did = HELD_BAD
        else:
            did = ADDED
            stats["added_in_kf"] += int(pML.is_in_keyframe(kf))
            pML.add_observation(kf, bi)                                # returns early when the line is in the keyframe already
            kf.slots[bi] = pML
        # the item's entry state was the live state and no earlier Replace of the item touched either line: the device's choice is the live one
        if first and jj == j and st >= 0 and st != UNRESOLVED and clean:
            assert st == did, (j, p, CODES[st], CODES[did])
            stats["checked"] += 1
        nFused += 1
    return nFused


def _null_repeats(lst):
    seen = set()
    return [(-1 if (p in seen or seen.add(p)) else p) if p >= 0 else -1 for p in lst]


def replay(g, prm, cur, targets, entry=None):
    """The caller's line half of SearchInNeighbors on the batched entries: two msl_fuse_map_lines calls (the targets sharing one list, then
    the current keyframe with msl_fuse_candidates' list), each replayed in order against the live objects, then the refresh of the current
    keyframe's lines.  Returns (rets, stats)."""
    entry = entry or ModelEntry()
    stats = dict(REPLACED_BY_HELD=0, REPLACES_HELD=0, SELF=0, researched=0, research_changed=0, UNRESOLVED=0, repeated=0, added_in_kf=0, checked=0)
    pCur = g.kfs[cur]
    rets = []
    orig = [-1 if s is None else s.id for s in pCur.slots]
    lines = g.lines()
    if targets:
        res = entry.fuse(prm, g.table(), lines, [(t, 0) for t in targets], [_null_repeats(orig)])
        for i, t in enumerate(targets):
            res[i]["_desc"] = lines["desc"]
            stats["UNRESOLVED"] += int((np.asarray(res[i]["status"]) == UNRESOLVED).sum())
            rets.append(_replay_item(g, prm, entry, g.kfs[t], orig, res[i], i == 0, stats))
    table, lines = g.table(), g.lines()
    cand = entry.candidates(table, lines, [list(targets)])[0]
    res = entry.fuse(prm, table, lines, [(cur, 0)], [cand])[0]
    res["_desc"] = lines["desc"]
    stats["UNRESOLVED"] += int((np.asarray(res["status"]) == UNRESOLVED).sum())
    rets.append(_replay_item(g, prm, entry, pCur, cand, res, True, stats))
    ids = []
    for s in pCur.slots:                                               # :609-618; a line in two slots is refreshed twice there, with one result
        if s is not None and not s.bad and s.id not in ids:
            ids.append(s.id)
    entry.refresh(g, prm, ids)
    return rets, stats

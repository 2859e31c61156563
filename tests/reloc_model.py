"""A literal, sequential CPU model of the keyframe search of Tracking::Relocalization:
ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*> &sAlreadyFound, th, ORBdist)
(reference src/ORBmatcher.cc:680-797) with MapPoint::PredictScale (src/MapPoint.cc:350-364), Frame::GetFeaturesInArea
(src/Frame.cc:332-381) and ComputeThreeMaxima (src/ORBmatcher.cc:799-830).

Test infrastructure only.  Float conventions are the ones DESIGN.md section 3 pins for the kernels (see tests/local_match_model.py, whose
gemm3 / predict_scale / features_in_area restatements are used here).  Inputs are the dicts of manhattanslam_amd.reloc.pack_keyframe_points.
The reference cannot be built here, so parity with it is unpinned: this model is the yardstick."""
import math

import numpy as np

from tests.bow_model import rot_bin, three_maxima
from tests.local_match_model import F32, features_in_area, gemm3, hamming, predict_scale

HISTO_LENGTH = 30                 # src/ORBmatcher.cc:35
POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.int64)


def project(p, T, xyz, dmin, dmax):
    """:702-734 for one map point: None (the loop's `continue`), or (u, v, level, radius).  p: a KEYFRAME_MATCH_PARAMS_DTYPE record."""
    fx, fy, cx, cy = (F32(p[k]) for k in ("fx", "fy", "cx", "cy"))
    minX, maxX, minY, maxY = (F32(p[k]) for k in ("minX", "maxX", "minY", "maxY"))
    tcw = T[:, 3]
    x3Dw = np.asarray(xyz, F32)
    x3Dc = gemm3(T, False, 1.0, x3Dw, tcw)                          # :703
    xc, yc = x3Dc[0], x3Dc[1]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        invzc = F32(np.float64(1.0) / np.float64(x3Dc[2]))          # :707: 1.0 / float, in double, rounded on assignment
        u = fx * xc * invzc + cx                                    # :709-710
        v = fy * yc * invzc + cy
    # The divergence from undefined behaviour: a non-finite u or v matches nothing.  (An infinity fails :712-715 in the reference as well;
    # a NaN passes there and is then cast to int inside GetFeaturesInArea.)
    if not (math.isfinite(float(u)) and math.isfinite(float(v))):
        return None
    if u < minX or u > maxX:                                        # :712  (no test of the sign of invzc)
        return None
    if v < minY or v > maxY:                                        # :714
        return None
    Ow = gemm3(T, True, -1.0, tcw)                                  # :686
    PO = x3Dw - Ow                                                  # :718, float32
    dist3D = F32(math.sqrt(sum(float(PO[k]) * float(PO[k]) for k in range(3))))   # :719 cv::norm
    maxDistance = F32(1.2) * F32(dmax)                              # :721-722
    minDistance = F32(0.8) * F32(dmin)
    if dist3D < minDistance or dist3D > maxDistance:                # :725
        return None
    level = predict_scale(dmax, dist3D, p["log_scale_factor"], int(p["nlevels"]))   # :728
    radius = F32(p["th"]) * F32(p["scale_factors"][level])         # :731
    return u, v, level, radius


def _grid(cur):
    grid = {}
    for i in range(len(cur["kps"])):
        c = int(cur["grid_cell"][i])
        if c >= 0:
            grid.setdefault(c, []).append(i)
    return grid


def search_keyframe_points(p, cur, kf, T, trace=None):
    """One pair.  Returns (match (N,) i32: the keyframe keypoint written into mvpMapPoints[i2] by this call, or -1; nmatches).
    trace (a dict, optional) receives what the non-vacuity conditions count: `unconstrained` (per query the pick it would make with nothing
    held at all, or -1), `pick` (its actual pick), `behind` (queries behind the camera that reach the window search), `culled` (matches the
    rotation check removed)."""
    p = p.reshape(-1)[0] if isinstance(p, np.ndarray) and p.shape else p
    T = np.asarray(T, F32)[:3, :4]
    n, m = len(cur["kps"]), len(kf["xyz"])
    orb_dist = int(p["orb_dist"])
    held = [bool(cur["held"][i]) for i in range(n)]                  # CurrentFrame.mvpMapPoints[i] != NULL
    match = [-1] * n
    grid = _grid(cur)
    rotHist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    tr = dict(unconstrained=[-1] * m, pick=[-1] * m, behind=0, culled=0)
    for i in range(m):                                              # :696
        if not (kf["flags"][i] & 1):                                # :699-700
            continue
        q = project(p, T, kf["xyz"][i], kf["dist"][i][0], kf["dist"][i][1])
        if q is None:
            continue
        u, v, level, radius = q
        if gemm3(T, False, 1.0, np.asarray(kf["xyz"][i], F32), T[:, 3])[2] < 0:
            tr["behind"] += 1
        idxs = features_in_area(p, grid, cur["kps"], cur["un_xy"], u, v, radius, level - 1, level + 1)   # :733
        if not idxs:                                                # :736
            continue
        bestDist, bestIdx2 = 256, -1
        freeDist, freeIdx = 256, -1
        dists = POPCOUNT[np.bitwise_xor(cur["desc"][idxs], kf["desc"][i])].sum(axis=1)   # DescriptorDistance of every candidate at once
        for i2, dist in zip(idxs, dists.tolist()):                  # :744-757
            if dist < freeDist:
                freeDist, freeIdx = dist, i2
            if held[i2]:                                            # :746
                continue
            if dist < bestDist:
                bestDist, bestIdx2 = dist, i2
        tr["unconstrained"][i] = freeIdx if freeDist <= orb_dist else -1
        if bestDist <= orb_dist:                                    # :759
            held[bestIdx2] = True                                   # :760
            match[bestIdx2] = i
            tr["pick"][i] = bestIdx2
            nmatches += 1
            if p["check_orientation"]:                              # :763-772
                b = rot_bin(kf["angle"][i], cur["kps"]["angle"][bestIdx2])
                assert 0 <= b < HISTO_LENGTH
                rotHist[b].append(bestIdx2)
    if p["check_orientation"]:                                      # :779-794
        keep = three_maxima([len(h) for h in rotHist])
        for b in range(HISTO_LENGTH):
            if b in keep:
                continue
            for i2 in rotHist[b]:
                match[i2] = -1
                nmatches -= 1
                tr["culled"] += 1
    if trace is not None:
        trace.update(tr)
    return np.array(match, np.int32), nmatches


def search_keyframe_points_fixpoint(p, cur, kf, T):
    """The same hand-out as the min-fixpoint the kernel solves (msl_assign.h with has_obs == true): t(i2) = the first query that picks
    keypoint i2 (-1 when held on entry), query i skips i2 iff t(i2) < i; iterate until nothing changes.  No rotation check.
    Returns the picks per query."""
    p = p.reshape(-1)[0] if isinstance(p, np.ndarray) and p.shape else p
    T = np.asarray(T, F32)[:3, :4]
    n, m = len(cur["kps"]), len(kf["xyz"])
    grid = _grid(cur)
    cands = []
    for i in range(m):
        c = []
        if kf["flags"][i] & 1:
            q = project(p, T, kf["xyz"][i], kf["dist"][i][0], kf["dist"][i][1])
            if q is not None:
                u, v, level, radius = q
                idxs = features_in_area(p, grid, cur["kps"], cur["un_xy"], u, v, radius, level - 1, level + 1)
                c = [(hamming(kf["desc"][i], cur["desc"][i2]), pos, i2) for pos, i2 in enumerate(idxs)]
        cands.append(c)
    FREE = 1 << 30
    seed = [-1 if cur["held"][i] else FREE for i in range(n)]
    pick = [-2] * m
    for _ in range(m + 2):
        t = list(seed)
        for i in range(m):
            if pick[i] >= 0:
                t[pick[i]] = min(t[pick[i]], i)
        new = []
        for i in range(m):
            free = [c for c in cands[i] if not t[c[2]] < i and c[0] < 256]
            best = min(free) if free else None
            new.append(best[2] if best is not None and best[0] <= int(p["orb_dist"]) else -1)
        if new == pick:
            break
        pick = new
    return pick


# ==== KeyFrameDatabase (reference src/KeyFrameDatabase.cc) ========================================================================================
def l1_score(v1, v2):
    """L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68) of two BowVectors given as (ascending words, double values): the
    merge walk, a sequential double sum in ascending word order, then -score / 2.0 (a double; the caller rounds it to float, :114)."""
    w1, x1 = v1
    w2, x2 = v2
    i = j = 0
    score = 0.0
    while i < len(w1) and j < len(w2):                              # :34
        if w1[i] == w2[j]:
            vi, wi = float(x1[i]), float(x2[j])
            score += math.fabs(vi - wi) - math.fabs(vi) - math.fabs(wi)   # :41
            i += 1; j += 1
        elif w1[i] < w2[j]:
            i += 1                                                  # lower_bound: the same element, reached one step at a time
        else:
            j += 1
    return -score / 2.0                                             # :65


class KeyFrame:
    """What DetectRelocalizationCandidates touches of a KeyFrame.  mRelocScore of a keyframe never scored is uninitialised in the
    reference; here it is 0.0f (the documented choice)."""

    def __init__(self, slot, words, values):
        self.slot, self.words, self.values = slot, [int(w) for w in words], [float(v) for v in values]
        self.mnRelocQuery, self.mnRelocWords, self.mRelocScore = -1, 0, F32(0.0)


class Database:
    """KeyFrameDatabase with its inverted file as lists (add :38-43, erase :45-61, clear :63-66).  Keyframes are named by their slot: the
    number of adds before them since the last clear."""

    def __init__(self):
        self.clear()

    def clear(self):
        self.inverted, self.kfs, self.query_id = {}, [], 0

    def add(self, words, values):
        kf = KeyFrame(len(self.kfs), words, values)
        self.kfs.append(kf)
        for w in kf.words:                                          # :41-42
            self.inverted.setdefault(w, []).append(kf)
        return kf.slot

    def erase(self, slot):
        kf = self.kfs[slot]
        for w in kf.words:                                          # :49-59
            lst = self.inverted[w]
            for k, other in enumerate(lst):
                if other is kf:
                    del lst[k]
                    break
        self.kfs[slot] = None

    def size(self):
        return len(self.kfs), sum(1 for k in self.kfs if k is not None)

    def detect(self, words, values, covis):
        """DetectRelocalizationCandidates (:68-170) for one frame.  covis[slot]: GetBestCovisibilityKeyFrames(10) as slots, in order.
        Returns (candidates as slots, mnRelocWords per slot (0 = shares no word), mRelocScore of this query per slot (-1 = not scored))."""
        self.query_id += 1
        fid = self.query_id
        n = len(self.kfs)
        words_out = np.zeros(n, np.int32); score_out = np.full(n, -1.0, np.float32)
        sharing = []
        for w in words:                                             # :75-88
            for kf in self.inverted.get(int(w), ()):
                if kf.mnRelocQuery != fid:
                    kf.mnRelocWords = 0
                    kf.mnRelocQuery = fid
                    sharing.append(kf)
                kf.mnRelocWords += 1
        for kf in sharing:
            words_out[kf.slot] = kf.mnRelocWords
        if not sharing:                                             # :90
            return [], words_out, score_out
        maxCommonWords = 0
        for kf in sharing:                                          # :94-99
            if kf.mnRelocWords > maxCommonWords:
                maxCommonWords = kf.mnRelocWords
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))        # :101
        lScoreAndMatch = []
        for kf in sharing:                                          # :108-118
            if kf.mnRelocWords > minCommonWords:
                si = F32(l1_score((list(words), list(values)), (kf.words, kf.values)))
                kf.mRelocScore = si
                score_out[kf.slot] = si
                lScoreAndMatch.append((si, kf))
        if not lScoreAndMatch:                                      # :120
            return [], words_out, score_out
        lAcc = []
        bestAccScore = F32(0)
        for si, kf in lScoreAndMatch:                               # :127-150
            bestScore = si
            accScore = bestScore
            pBestKF = kf
            for s2 in covis[kf.slot][:10]:
                if s2 < 0 or s2 >= n or self.kfs[s2] is None:       # a culled keyframe is in no list: its mnRelocQuery differs
                    continue
                kf2 = self.kfs[s2]
                if kf2.mnRelocQuery != fid:                         # :137
                    continue
                accScore = F32(accScore + kf2.mRelocScore)          # :140
                if kf2.mRelocScore > bestScore:
                    pBestKF = kf2
                    bestScore = kf2.mRelocScore
            lAcc.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        minScoreToRetain = F32(0.75) * bestAccScore                 # :153
        added, out = set(), []
        for si, kf in lAcc:                                         # :157-167
            if si > minScoreToRetain and kf.slot not in added:
                out.append(kf.slot)
                added.add(kf.slot)
        return out, words_out, score_out


def detect_by_keys(db, words, values, covis):
    """The independent formulation the kernels use: per slot the number of shared words, the first shared word and the score by direct
    intersection; the sharing list as the sort of (first shared word, slot).  Reads db's scores without changing them.  Returns the
    candidates."""
    qs = {int(w): float(v) for w, v in zip(words, values)}
    n = len(db.kfs)
    cnt, first = [0] * n, [None] * n
    for s, kf in enumerate(db.kfs):
        if kf is None:
            continue
        common = [w for w in kf.words if w in qs]
        cnt[s], first[s] = len(common), (min(common) if common else None)
    if not any(cnt):
        return []
    mn = int(F32(max(cnt)) * F32(0.8))
    order = sorted((first[s], s) for s in range(n) if cnt[s] > mn)
    score = [db.kfs[s].mRelocScore if db.kfs[s] is not None else F32(0) for s in range(n)]
    for _, s in order:
        kf = db.kfs[s]
        tot = 0.0
        for w, v in zip(kf.words, kf.values):                       # ascending keyframe words = ascending common words
            if w in qs:
                tot += math.fabs(qs[w] - v) - math.fabs(qs[w]) - math.fabs(v)
        score[s] = F32(-tot / 2.0)
    acc = []
    for _, s in order:
        a, best, bk = score[s], score[s], s
        for s2 in covis[s][:10]:
            if 0 <= s2 < n and cnt[s2] > 0:
                a = F32(a + score[s2])
                if score[s2] > best:
                    best, bk = score[s2], s2
        acc.append((a, bk))
    top = max([F32(0)] + [a for a, _ in acc])
    out = []
    for a, bk in acc:
        if a > F32(0.75) * top and bk not in out:
            out.append(bk)
    return out

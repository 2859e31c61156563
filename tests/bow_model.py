"""A literal, sequential CPU model of the bag-of-words layer, the parity reference of msl_bow_transform, msl_match_by_bow and
msl_match_lines_by_descriptor (and of msl_vocab_load_text).  Written from the behaviour of DBoW2's TemplatedVocabulary
(loadFromTextFile, transform; reference Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h), ORBmatcher::SearchByBoW(KeyFrame*, Frame&)
(src/ORBmatcher.cc:146-247, ComputeThreeMaxima :799-830) and LSDmatcher::SearchByDescriptor (src/LSDmatcher.cpp:201-234).

Test infrastructure only.  A vocabulary is the dict build() returns: node arrays over nodes 0 .. n - 1 (node 0 the root), children lists in
file order, word ids of the flagged nodes in file order (0 for every other node).  Types as the reference has them: Hamming distances are
ints compared as doubles (the same order), the BowVector is a std::map of doubles summed in feature order and normalised in ascending word
order, the matchers' ratio tests are float expressions.

Two definitions where the reference is undefined (documented in INTEGRATION.md):
  * the descent stopping above level L - levelsup leaves nid unset in the reference; here nid is the node where it stopped;
  * SearchByDescriptor with no keyframe line or fewer than two current lines reads past a vector; here it matches nothing.
And one deliberate loader divergence: blank lines are skipped (the reference turns a trailing newline into an extra childless root child)."""
import math

import numpy as np

F32 = np.float32
TF_IDF, TF, IDF, BINARY = range(4)
L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT = range(6)
TH_LOW, HISTO_LENGTH = 50, 30
POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.int64)


def hamming(a, b):
    """FORB::distance / ORBmatcher::DescriptorDistance / LSDmatcher::DescriptorDistance: popcount of a ^ b over 256 bits."""
    return int(POPCOUNT[np.bitwise_xor(np.asarray(a, np.uint8), np.asarray(b, np.uint8))].sum())


def build(k, L, scoring, weighting, parent, is_leaf, desc, weight):
    """The node table loadFromTextFile builds (entry 0 of every array is the root and is not read)."""
    parent = np.asarray(parent, np.int64)
    n = len(parent)
    children = [[] for _ in range(n)]
    word_id = np.zeros(n, np.int64)
    nw = 0
    for i in range(1, n):
        assert 0 <= parent[i] < i
        children[parent[i]].append(i)
        if is_leaf[i]:
            word_id[i] = nw
            nw += 1
    return {"k": k, "L": L, "scoring": scoring, "weighting": weighting, "children": children, "word_id": word_id, "n_words": nw,
            "desc": np.asarray(desc, np.uint8).reshape(n, 32), "weight": np.asarray(weight, np.float64).reshape(n)}


def load_text(text):
    """The text loader: header "k L scoring weighting", then "parent isLeaf d0..d31 weight" per node; blank lines skipped.  Returns the
    argument tuple of build() or None where the loader refuses."""
    lines = text.split("\n")
    head = lines[0].split()
    if len(head) < 4:
        return None
    k, L, sc, wt = (int(x) for x in head[:4])
    if not (2 <= k <= 20 and 1 <= L <= 10 and 0 <= sc <= 5 and 0 <= wt <= 3):
        return None
    parent, leaf, desc, weight = [0], [0], [[0] * 32], [0.0]
    for ln in lines[1:]:
        if not ln.strip():
            continue
        t = ln.split()
        parent.append(int(t[0]))
        leaf.append(1 if int(t[1]) > 0 else 0)
        desc.append([int(x) & 0xFF for x in t[2:34]])
        weight.append(float(t[34]))
    return k, L, sc, wt, np.array(parent), np.array(leaf, np.uint8), np.array(desc, np.uint8), np.array(weight)


def write_text(k, L, scoring, weighting, parent, is_leaf, desc, weight, trailing_newline=True):
    """saveToTextFile's layout (weights printed exactly: repr round-trips a double)."""
    rows = [f"{k} {L} {scoring} {weighting}"]
    desc = np.asarray(desc, np.uint8)
    for i in range(1, len(parent)):
        rows.append(f"{int(parent[i])} {1 if is_leaf[i] else 0} " + " ".join(str(int(x)) for x in desc[i]) + f" {float(weight[i])!r}")
    return "\n".join(rows) + ("\n" if trailing_newline else "")


def descend(V, d, levelsup):
    """transform(feature, word_id, weight, &nid, levelsup): returns (word_id, weight, nid)."""
    nid_level = V["L"] - levelsup
    nid = 0 if nid_level <= 0 else None
    final_id, level = 0, 0
    while True:
        level += 1
        nodes = V["children"][final_id]
        final_id = nodes[0]
        best_d = float(hamming(d, V["desc"][final_id]))
        for c in nodes[1:]:
            dd = float(hamming(d, V["desc"][c]))
            if dd < best_d:
                best_d, final_id = dd, c
        if level == nid_level:
            nid = final_id
        if not V["children"][final_id]:       # isLeaf(): no children
            break
    if nid is None:
        nid = final_id                         # defined here: the reference leaves nid uninitialised
    return int(V["word_id"][final_id]), float(V["weight"][final_id]), nid


def normalize(bow, scoring):
    """BowVector::normalize for the scoring's LNorm (every scoring but DOT_PRODUCT), in ascending word order."""
    norm = 0.0
    if scoring == L2_NORM:
        for w in sorted(bow):
            norm += bow[w] * bow[w]
        norm = math.sqrt(norm)
    else:
        for w in sorted(bow):
            norm += abs(bow[w])
    if norm > 0.0:
        for w in sorted(bow):
            bow[w] /= norm


def transform(V, descs, levelsup):
    """transform(features, BowVector, FeatureVector, levelsup).  Returns (word [N], node [N] (-1 = stopped), bow {word: value}, fv {node: [i]})."""
    n = len(descs)
    word, node = [-1] * n, [-1] * n
    bow, fv = {}, {}
    if V["n_words"] == 0:                      # empty(): nothing at all
        return word, node, bow, fv
    tf = V["weighting"] in (TF, TF_IDF)
    must = V["scoring"] != DOT_PRODUCT
    for i, d in enumerate(descs):
        wid, w, nid = descend(V, d, levelsup)
        if w > 0:
            if tf:
                bow[wid] = bow[wid] + w if wid in bow else w      # addWeight
            elif wid not in bow:
                bow[wid] = w                                     # addIfNotExist
            fv.setdefault(nid, []).append(i)
            word[i], node[i] = wid, nid
    if tf and bow and not must:
        nd = float(len(bow))
        for w in sorted(bow):
            bow[w] /= nd
    if must:
        normalize(bow, V["scoring"])
    return word, node, dict(sorted(bow.items())), dict(sorted(fv.items()))


def rot_bin(a_kf, a_f):
    """The histogram bin of rot = kp.angle - F.mvKeys[i].angle (float), or -1 outside [0, HISTO_LENGTH)."""
    rot = F32(F32(a_kf) - F32(a_f))
    if rot < 0.0:
        rot = F32(rot + F32(360.0))
    x = F32(rot * F32(1.0 / HISTO_LENGTH))
    b = int(math.floor(float(x) + 0.5))        # round(): half away from zero, x >= 0
    if b == HISTO_LENGTH:
        b = 0
    return b if 0 <= b < HISTO_LENGTH else -1


def three_maxima(counts):
    """ComputeThreeMaxima on the bin sizes."""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(counts):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2, ind3, ind2 = max2, s, ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if F32(max2) < F32(0.1) * F32(max1):
        ind2 = ind3 = -1
    elif F32(max3) < F32(0.1) * F32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def search_by_bow(p, nn_ratio=0.7, check_orientation=True):
    """SearchByBoW(pKF, F, vpMapPointMatches) on a pair dict of manhattanslam_amd.bow.  Returns (match [n_cur]: keyframe index or -1, nmatches)."""
    nkf, ncur = len(p["kf_desc"]), len(p["cur_desc"])
    fv_kf, fv_f = {}, {}
    for i in range(nkf):
        if p["kf_node"][i] >= 0:
            fv_kf.setdefault(int(p["kf_node"][i]), []).append(i)
    for i in range(ncur):
        if p["cur_node"][i] >= 0:
            fv_f.setdefault(int(p["cur_node"][i]), []).append(i)
    match = [-1] * ncur
    hist = [[] for _ in range(HISTO_LENGTH)]
    nm = 0
    ratio = F32(nn_ratio)
    for nd in sorted(set(fv_kf) & set(fv_f)):          # the merge walk visits the common nodes in ascending order
        cand = np.array(fv_f[nd])
        cdesc = np.asarray(p["cur_desc"], np.uint8)[cand]
        for iKF in fv_kf[nd]:
            if not (p["kf_flags"][iKF] & 1):
                continue
            # the candidate loop over vIndicesF (ascending), distances computed at once: skip the matched, then
            # `d < bestDist1` keeps the first minimum and `d < bestDist2` the second smallest value, both starting at 256
            dist = POPCOUNT[np.bitwise_xor(cdesc, np.asarray(p["kf_desc"][iKF], np.uint8))].sum(axis=1)
            free = np.array([match[i] < 0 for i in cand], bool)
            ds, ids = dist[free], cand[free]
            best1, best_idx, best2 = 256, -1, 256
            if len(ds):
                j = int(np.argmin(ds))
                if ds[j] < 256:
                    best1, best_idx = int(ds[j]), int(ids[j])
                    rest = np.delete(ds, j)
                    best2 = int(min(256, rest.min())) if len(rest) else 256
            if best1 <= TH_LOW and F32(best1) < ratio * F32(best2):
                match[best_idx] = iKF
                if check_orientation:
                    b = rot_bin(p["kf_angle"][iKF], p["cur_angle"][best_idx])
                    assert b >= 0
                    hist[b].append(best_idx)
                nm += 1
    if check_orientation:
        keep = three_maxima([len(h) for h in hist])
        for i in range(HISTO_LENGTH):
            if i in keep:
                continue
            for iF in hist[i]:
                match[iF] = -1
                nm -= 1
    return match, nm


def knn2(kf_ldesc, cur_ldesc):
    """BFMatcher(NORM_HAMMING).knnMatch(kf, cur, lmatches, 2): per query the two first entries of the (distance, train index) insertion
    order -- a later equal distance never displaces an earlier one."""
    out = []
    for q in range(len(kf_ldesc)):
        best = []                                       # [(dist, train)] at most two, kept in insertion order
        for t in range(len(cur_ldesc)):
            d = hamming(kf_ldesc[q], cur_ldesc[t])
            if len(best) < 2 or d < best[-1][0]:
                pos = len(best)
                while pos > 0 and d < best[pos - 1][0]:
                    pos -= 1
                best.insert(pos, (d, t))
                best = best[:2]
        out.append(best)
    return out


def search_by_descriptor(p):
    """SearchByDescriptor(pKF, currentF, vpMapLineMatches).  Returns (match [n_cur]: the last keyframe line written, or -1, nmatches)."""
    nkf, ncur = len(p["kf_ldesc"]), len(p["cur_ldesc"])
    match = [-1] * ncur
    if nkf == 0 or ncur < 2:                            # defined here: the reference reads past a vector's end
        return match, 0
    nm = 0
    min_ratio = F32(F32(1.0) / F32(1.5))
    for q, m in enumerate(knn2(p["kf_ldesc"], p["cur_ldesc"])):
        with np.errstate(invalid="ignore", divide="ignore"):
            r = F32(m[0][0]) / F32(m[1][0])
        if r < min_ratio and (p["kf_flags"][q] & 1):
            match[m[0][1]] = q
            nm += 1
    return match, nm

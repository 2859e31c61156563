"""The bag-of-words CPU model against independent formulations, and hand-built cases pinning each quirk of the reference (no GPU)."""
import collections
import math

import numpy as np
import pytest

from tests import bow_model as M
from tests import bow_scenes as S


def brute_descend(V, d, levelsup):
    """Full-path descent with numpy: per level every child's distance at once, np.argmin = the first minimum."""
    path, node = [0], 0
    while V["children"][node]:
        ch = np.array(V["children"][node])
        dist = M.POPCOUNT[np.bitwise_xor(V["desc"][ch], d)].sum(axis=1)
        node = int(ch[np.argmin(dist)])
        path.append(node)
    lvl = V["L"] - levelsup
    nid = 0 if lvl <= 0 else (path[lvl] if lvl < len(path) else path[-1])
    return int(V["word_id"][node]), float(V["weight"][node]), nid


def counter_transform(V, descs, levelsup):
    """BowVector as a per-word Counter of weights in feature order (TF / TF_IDF) or the first weight (IDF / BINARY)."""
    if V["n_words"] == 0:
        return {}
    res = [brute_descend(V, d, levelsup) for d in descs]
    kept = [(w, x) for w, x, _ in res if x > 0]
    if V["weighting"] in (M.TF, M.TF_IDF):
        acc = collections.OrderedDict()
        for w, x in kept:
            acc[w] = acc[w] + x if w in acc else x
        bow = dict(acc)
        if V["scoring"] == M.DOT_PRODUCT and bow:
            bow = {w: x / float(len(bow)) for w, x in bow.items()}
    else:
        firsts = collections.Counter()
        bow = {}
        for w, x in kept:
            if not firsts[w]:
                bow[w] = x
            firsts[w] += 1
    if V["scoring"] != M.DOT_PRODUCT:
        keys = sorted(bow)
        norm = math.sqrt(sum(bow[w] * bow[w] for w in keys)) if V["scoring"] == M.L2_NORM else sum(abs(bow[w]) for w in keys)
        if norm > 0:
            bow = {w: bow[w] / norm for w in keys}
    return dict(sorted(bow.items()))


@pytest.mark.parametrize("seed", range(6))
def test_descent_and_bow_vector_match_brute_force(seed):
    for wt in range(4):
        for sc in range(6):
            V = M.build(*S.random_vocab(seed * 31 + wt * 7 + sc, k=3 + seed % 5, L=2 + seed % 4, scoring=sc, weighting=wt))
            descs = S.frame_descs(seed + 100, (0, 0, 0, 0, None, None, V["desc"]), 60)
            for levelsup in (0, 1, 2, V["L"], V["L"] + 1):
                word, node, bow, fv = M.transform(V, descs, levelsup)
                ref = [brute_descend(V, d, levelsup) for d in descs]
                if V["n_words"]:
                    assert word == [w if x > 0 else -1 for w, x, _ in ref]
                    assert node == [n if x > 0 else -1 for _, x, n in ref]
                assert bow == counter_transform(V, descs, levelsup)
                assert fv == {nd: [i for i in range(len(descs)) if node[i] == nd] for nd in set(node) - {-1}}


def _tiny(descs_children, weights, flags, parents, k=4, L=2, sc=M.DOT_PRODUCT, wt=M.TF_IDF):
    n = len(parents)
    d = np.zeros((n, 32), np.uint8)
    for i, v in descs_children.items():
        d[i] = v
    return M.build(k, L, sc, wt, np.array(parents), np.array(flags, np.uint8), d, np.array(weights, float))


def test_ties_go_to_the_earliest_child_and_leaf_means_childless():
    # root -> 1, 2 (equal descriptors) ; 1 -> 3 (flagged) ; 2 -> 4 ; node 2 also flagged but has a child
    V = _tiny({1: 0xF0, 2: 0xF0, 3: 0, 4: 0}, [0, 1, 1, 2.5, 3.5], [0, 0, 1, 1, 1], [0, 0, 0, 1, 2])
    wid, w, nid = M.descend(V, np.zeros(32, np.uint8), 0)
    assert (wid, w, nid) == (int(V["word_id"][3]), 2.5, 3)      # child 1 wins the tie, the descent continues past flagged nodes with children
    assert V["word_id"][2] == 0 and V["word_id"][3] == 1 and V["word_id"][4] == 2


def test_unflagged_childless_node_keeps_word_zero_and_its_weight():
    V = _tiny({1: 0, 2: 0xFF}, [0, 0.75, 2.0], [0, 0, 1], [0, 0, 0], L=1)
    assert M.descend(V, np.zeros(32, np.uint8), 0) == (0, 0.75, 1)
    # two nodes share word id 0 with different weights: TF sums them in feature order, IDF keeps the first
    desc = np.array([np.zeros(32), np.full(32, 0xFF)], np.uint8)
    for wt, expect in ((M.TF, (0.75 + 2.0) / 1), (M.IDF, 0.75)):
        V["weighting"] = wt
        assert M.transform(V, desc, 0)[2] == {0: expect}
    V["weighting"] = M.IDF
    assert M.transform(V, desc[::-1], 0)[2] == {0: 2.0}


def test_sequential_sum_is_not_a_product():
    V = _tiny({1: 0}, [0, 0.1], [0, 1], [0, 0], L=1, wt=M.TF)
    bow = M.transform(V, np.zeros((10, 32), np.uint8), 0)[2]
    s = 0.1
    for _ in range(9):
        s += 0.1
    assert bow == {0: s} and s != 10 * 0.1


def test_node_level_root_and_stop_above():
    # chain root -> 1 -> 2 (flagged) and root -> 3 (flagged, shallow), L = 3
    V = _tiny({1: 0, 2: 0, 3: 0xFF}, [0, 1, 1, 1], [0, 0, 1, 1], [0, 0, 1, 0], L=3)
    z, o = np.zeros(32, np.uint8), np.full(32, 0xFF, np.uint8)
    assert M.descend(V, z, 3)[2] == 0 and M.descend(V, z, 5)[2] == 0         # L - levelsup <= 0: the root
    assert M.descend(V, z, 2)[2] == 1 and M.descend(V, z, 1)[2] == 2
    assert M.descend(V, z, 0)[2] == 2                                          # level 3 never reached: the stopped node
    assert M.descend(V, o, 1)[2] == 3


def test_stopped_words_and_empty_vocabulary():
    V = _tiny({1: 0, 2: 0xFF}, [0, 0.0, 1.0], [0, 1, 1], [0, 0, 0], L=1, sc=M.L1_NORM)
    word, node, bow, fv = M.transform(V, np.array([np.zeros(32), np.full(32, 0xFF)], np.uint8), 0)
    assert word == [-1, 1] and node == [-1, 2] and bow == {1: 1.0} and fv == {2: [1]}
    E = _tiny({1: 0}, [0, 1.0], [0, 0], [0, 0], L=1)
    assert M.transform(E, np.zeros((3, 32), np.uint8), 0) == ([-1] * 3, [-1] * 3, {}, {})


def test_normalisations():
    V = _tiny({1: 0, 2: 0xFF}, [0, 3.0, 4.0], [0, 1, 1], [0, 0, 0], L=1)
    desc = np.array([np.zeros(32), np.full(32, 0xFF), np.full(32, 0xFF)], np.uint8)
    for sc, wt, expect in ((M.L2_NORM, M.TF_IDF, {0: 3 / math.sqrt(9 + 64), 1: 8 / math.sqrt(9 + 64)}), (M.L1_NORM, M.TF, {0: 3 / 11, 1: 8 / 11}),
                           (M.DOT_PRODUCT, M.TF, {0: 1.5, 1: 4.0}), (M.DOT_PRODUCT, M.BINARY, {0: 3.0, 1: 4.0}),
                           (M.CHI_SQUARE, M.IDF, {0: 3 / 7, 1: 4 / 7})):
        V["scoring"], V["weighting"] = sc, wt
        assert M.transform(V, desc, 0)[2] == expect


def test_loader_round_trip_and_refusals():
    args = S.random_vocab(5, k=4, L=3)
    V0 = M.build(*args)
    for trailing in (True, False):
        got = M.load_text(M.write_text(*args, trailing_newline=trailing))
        assert got[:4] == args[:4]
        for a, b in zip(got[4:], args[4:]):
            assert np.array_equal(a[1:], b[1:])                        # entry 0, the root, is not part of the file
        V1 = M.build(*got)
        assert V1["children"] == V0["children"] and np.array_equal(V1["word_id"], V0["word_id"])
    for head in ("1 3 0 0", "21 3 0 0", "4 0 0 0", "4 11 0 0", "4 3 6 0", "4 3 0 4", "-1 3 0 0"):
        assert M.load_text(head + "\n0 1 " + "0 " * 32 + "1\n") is None


def dict_search_by_bow(p, nn_ratio, check_orientation):
    """SearchByBoW from the FeatureVector maps: the merge walk over two sorted maps, per-node lists, sorted candidate distances."""
    fk, ff = collections.defaultdict(list), collections.defaultdict(list)
    for i, nd in enumerate(p["kf_node"]):
        if nd >= 0:
            fk[int(nd)].append(i)
    for i, nd in enumerate(p["cur_node"]):
        if nd >= 0:
            ff[int(nd)].append(i)
    holder = {}
    kept = []
    for nd in sorted(fk):
        if nd not in ff:
            continue
        for iKF in fk[nd]:
            if not p["kf_flags"][iKF] & 1:
                continue
            cands = sorted((M.hamming(p["kf_desc"][iKF], p["cur_desc"][iF]), iF) for iF in ff[nd] if iF not in holder)
            d1 = cands[0][0] if cands and cands[0][0] < 256 else 256
            d2 = cands[1][0] if len(cands) > 1 else 256
            if d1 <= 50 and np.float32(d1) < np.float32(nn_ratio) * np.float32(d2):
                holder[cands[0][1]] = iKF
                kept.append(cands[0][1])
    if check_orientation:
        bins = {iF: M.rot_bin(p["kf_angle"][holder[iF]], p["cur_angle"][iF]) for iF in kept}
        keep = M.three_maxima([sum(1 for b in bins.values() if b == i) for i in range(30)])
        for iF, b in bins.items():
            if b not in keep:
                del holder[iF]
    return [holder.get(i, -1) for i in range(len(p["cur_desc"]))], len(holder)


@pytest.mark.parametrize("seed", range(8))
def test_search_by_bow_matches_the_map_formulation(seed):
    p = S.bow_pair(seed, 40 + seed * 15, 50 + seed * 12, n_nodes=3 + seed)
    for ratio, orient in ((0.7, True), (0.75, True), (0.9, False)):
        m, n = M.search_by_bow(p, ratio, orient)
        assert (m, n) == dict_search_by_bow(p, ratio, orient)
        assert n == sum(1 for x in m if x >= 0)


def test_search_by_bow_pins():
    z = np.zeros(32, np.uint8)
    one = z.copy(); one[0] = 1
    base = {"kf_angle": np.zeros(2, np.float32), "kf_node": np.array([7, 7], np.int32), "kf_flags": np.array([1, 1], np.uint8),
            "cur_node": np.array([7, 7, 7], np.int32), "cur_angle": np.zeros(3, np.float32)}
    # a tie (bestDist2 == bestDist1) is rejected; the first frame feature is the best on a tie
    p = dict(base, kf_desc=np.array([z, one]), cur_desc=np.array([z, z, np.full(32, 0xFF, np.uint8)]))
    assert M.search_by_bow(p, 0.7, False) == ([-1, -1, -1], 0)
    # keyframe 0 takes frame 0; keyframe 1 then skips it (in-node exclusion) and must take frame 1
    p = dict(base, kf_desc=np.array([z, z]), cur_desc=np.array([z, np.full(32, 0x0F, np.uint8), np.full(32, 0xFF, np.uint8)]))
    assert M.search_by_bow(p, 0.7, False) == ([0, -1, -1], 1)
    p["cur_desc"][1] = one
    assert M.search_by_bow(p, 0.7, False) == ([0, 1, -1], 2)
    # bins: only 0..12 occur (rot * (1/30) rounded, 360 -> bin 12); 0.1f * max1 cut
    assert M.rot_bin(359.0, 0.0) == 12 and M.rot_bin(0.0, 1.0) == 12 and M.rot_bin(14.9, 0.0) == 0 and M.rot_bin(15.0, 0.0) == 1
    assert M.three_maxima([10, 1, 0, 2] + [0] * 26) == (0, 3, 1)
    assert M.three_maxima([20, 1, 0, 2] + [0] * 26) == (0, 3, -1)
    assert M.three_maxima([30, 1, 0, 2] + [0] * 26) == (0, -1, -1)


def argsort_search_by_descriptor(p):
    nkf, ncur = len(p["kf_ldesc"]), len(p["cur_ldesc"])
    if nkf == 0 or ncur < 2:
        return [-1] * ncur, 0
    D = np.array([[M.hamming(a, b) for b in p["cur_ldesc"]] for a in p["kf_ldesc"]])
    order = np.argsort(D, axis=1, kind="stable")
    match, nm = [-1] * ncur, 0
    for q in range(nkf):
        d0, d1 = D[q, order[q, 0]], D[q, order[q, 1]]
        with np.errstate(invalid="ignore", divide="ignore"):
            ok = np.float32(d0) / np.float32(d1) < np.float32(1 / 1.5)
        if ok and p["kf_flags"][q] & 1:
            match[order[q, 0]] = q
            nm += 1
    return match, nm


@pytest.mark.parametrize("seed", range(8))
def test_search_by_descriptor_matches_argsort(seed):
    p = S.line_pair(seed, [0, 1, 5, 30, 60, 3, 40, 25][seed], [7, 1, 2, 30, 45, 0, 64, 25][seed])
    assert M.search_by_descriptor(p) == argsort_search_by_descriptor(p)


def test_search_by_descriptor_pins():
    z = np.zeros(32, np.uint8)
    a, b = z.copy(), z.copy()
    a[0], b[1] = 1, 3
    # knn order: equal distances keep the lower train index first, so a tie is a ratio of 1 (rejected)
    assert M.knn2([z], [a, z, z]) == [[(0, 1), (0, 2)]]
    assert M.search_by_descriptor({"kf_ldesc": [z], "kf_flags": [1], "cur_ldesc": [a, z, z]}) == ([-1, -1, -1], 0)
    # 0 / x accepted; later queries overwrite earlier ones and every write counts; a line without a map line is skipped
    p = {"kf_ldesc": [z, z, z], "kf_flags": [1, 0, 1], "cur_ldesc": [b, z, np.full(32, 0xFF, np.uint8)]}
    assert M.search_by_descriptor(p) == ([-1, 2, -1], 2)
    # ratio exactly 2/3 is not below (float)(1/1.5)
    c = z.copy(); c[0] = 0x03
    d = z.copy(); d[0] = 0x07
    assert M.search_by_descriptor({"kf_ldesc": [z], "kf_flags": [1], "cur_ldesc": [c, d]}) == ([-1, -1], 0)
    e = z.copy(); e[0] = 0x0F
    assert M.search_by_descriptor({"kf_ldesc": [z], "kf_flags": [1], "cur_ldesc": [c, e]}) == ([0, -1], 1)
    # undefined in the reference, defined here
    assert M.search_by_descriptor({"kf_ldesc": [], "kf_flags": [], "cur_ldesc": [z, z]}) == ([-1, -1], 0)
    assert M.search_by_descriptor({"kf_ldesc": [z], "kf_flags": [1], "cur_ldesc": [z]}) == ([-1], 0)

"""The CPU model of the keyframe search (tests/reloc_model.py) against independent formulations and hand-built cases, one per quirk of
ORBmatcher::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist) (src/ORBmatcher.cc:680-797); and the conditions under which
the generated GPU scenes (tests/reloc_scenes.py) are not vacuous.  No GPU."""
import math

import numpy as np
import pytest

from tests import reloc_model as rm
from tests import reloc_scenes as rs

I4 = np.eye(4, dtype=np.float32)


def _range(dist, level, scale=1.2, nlevels=8):
    """(mfMinDistance, mfMaxDistance) that predicts `level` at distance dist."""
    dmax = dist * scale ** (level - 0.5)
    return (dmax / scale ** (nlevels - 1), dmax)


def _point(p, u, v, z, level=0, angle=0.0, flags=1):
    xyz = rs.pixel_point(p, u, v, z)
    return (xyz, _range(math.sqrt(sum(c * c for c in xyz)), level), angle, flags)


@pytest.mark.parametrize("seed,kw", [(1, {}), (2, dict(conflict=True)), (3, dict(cluster=True, held=0.5)), (4, dict(identity=True))])
def test_literal_loop_equals_the_min_fixpoint(seed, kw):
    """The hand-out as the reference's pointer loop against the fixpoint the kernel solves, on random pairs without the rotation check."""
    p = rs.params(10.0, 100, check_orientation=False)
    cur, kf, T = rs.random_pair(seed, p, n_cur=250, n_kf=300, **kw)
    tr = {}
    match, nm = rm.search_keyframe_points(p, cur, kf, T, tr)
    pick = rm.search_keyframe_points_fixpoint(p, cur, kf, T)
    assert pick == tr["pick"] and nm == sum(1 for x in pick if x >= 0) and nm > 20
    want = np.full(len(match), -1, np.int32)
    for q, i2 in enumerate(pick):
        if i2 >= 0:
            assert want[i2] == -1                                   # nothing is ever overwritten
            want[i2] = q
    assert np.array_equal(match, want) and not np.any(match[cur["held"] != 0] >= 0)


def test_a_point_behind_the_camera_matches():
    """There is no positive-depth test: the point at -z on the keypoint's ray projects onto the keypoint and takes it."""
    p = rs.params(3.0, 64, False)
    cur = rs.frame(p, [(200.0, 150.0, 0, 0, 0.0, 0)])
    kf = rs.keyframe([_point(p, 200.0, 150.0, -2.0)])
    tr = {}
    match, nm = rm.search_keyframe_points(p, cur, kf, I4, tr)
    assert nm == 1 and match.tolist() == [0] and tr["behind"] == 1


def test_depth_zero_matches_nothing():
    """zc == 0: an infinite projection fails the bounds test as in the reference; a NaN one (xc == 0 too) would pass it there and reach an
    undefined float-to-int conversion -- here it matches nothing (the documented divergence)."""
    p = rs.params(10.0, 100, False)
    cur = rs.frame(p, [(float(p["cx"][0]), float(p["cy"][0]), 0, 0, 0.0, 0), (10.0, 10.0, 0, 0, 0.0, 0)])
    for xyz in ((0.0, 0.0, 0.0), (0.5, 0.0, 0.0), (0.0, -0.5, 0.0)):
        kf = rs.keyframe([(xyz, (0.0, 100.0), 0.0, 1)])
        assert rm.project(p.reshape(-1)[0], I4[:3], xyz, 0.0, 100.0) is None
        match, nm = rm.search_keyframe_points(p, cur, kf, I4)
        assert nm == 0 and np.all(match == -1)


def test_every_candidate_held_gives_no_match():
    p = rs.params(10.0, 100, False)
    cur = rs.frame(p, [(200.0, 150.0, 0, 0, 0.0, 1), (202.0, 151.0, 0, 3, 0.0, 1)])
    kf = rs.keyframe([_point(p, 200.0, 150.0, 2.0)])
    match, nm = rm.search_keyframe_points(p, cur, kf, I4)
    assert nm == 0 and np.all(match == -1)


def test_an_earlier_query_takes_a_later_querys_best():
    """Two points on one keypoint: the first takes it, the second falls back to its second choice (and a third gets nothing)."""
    p = rs.params(10.0, 100, False)
    cur = rs.frame(p, [(200.0, 150.0, 0, 0, 0.0, 0), (203.0, 150.0, 0, 40, 0.0, 0)])
    kf = rs.keyframe([_point(p, 200.0, 150.0, 2.0), _point(p, 200.5, 150.0, 2.5), _point(p, 201.0, 150.0, 3.0)])
    tr = {}
    match, nm = rm.search_keyframe_points(p, cur, kf, I4, tr)
    assert match.tolist() == [0, 1] and nm == 2 and tr["pick"] == [0, 1, -1] and tr["unconstrained"] == [0, 0, 0]


def test_distance_exactly_orb_dist_is_accepted_one_more_is_not():
    p = rs.params(10.0, 64, False)
    kf = rs.keyframe([_point(p, 200.0, 150.0, 2.0)])
    assert rm.search_keyframe_points(p, rs.frame(p, [(200.0, 150.0, 0, 64, 0.0, 0)]), kf, I4)[1] == 1
    assert rm.search_keyframe_points(p, rs.frame(p, [(200.0, 150.0, 0, 65, 0.0, 0)]), kf, I4)[1] == 0


def test_first_minimum_in_walk_order_wins_a_tie():
    """Equal distances: the walk goes by cell column, then row, then insertion order, and `dist < bestDist` keeps the first."""
    p = rs.params(10.0, 100, False)
    cur = rs.frame(p, [(206.0, 150.0, 0, 5, 0.0, 0), (194.0, 158.0, 0, 5, 0.0, 0), (194.0, 142.0, 0, 5, 0.0, 0)])
    match, nm = rm.search_keyframe_points(p, cur, rs.keyframe([_point(p, 200.0, 150.0, 2.0)]), I4)
    assert nm == 1 and match.tolist() == [-1, -1, 0]                # cell column 19, row 14 comes first


def test_level_is_clamped_at_both_ends():
    """PredictScale: a ratio beyond the pyramid clamps to nlevels - 1; a negative level (reachable inside the distance range when
    log_scale_factor < log 1.2) clamps to 0."""
    p = rs.params(10.0, 100, False).reshape(-1)[0]
    xyz = rs.pixel_point(rs.params(), 200.0, 150.0, 2.0)
    d = math.sqrt(sum(c * c for c in xyz))
    u, v, level, radius = rm.project(p, I4[:3], xyz, 0.0, d * 1.2 ** 12)
    assert level == 7 and radius == np.float32(10.0) * p["scale_factors"][7]
    p11 = rs.params(10.0, 100, False, scale=1.1).reshape(-1)[0]
    assert rm.predict_scale(d / 1.15, np.float32(d), p11["log_scale_factor"], 8) == 0
    assert math.ceil(math.log(1 / 1.15) / math.log(1.1)) == -1       # the unclamped level
    u, v, level, radius = rm.project(p11, I4[:3], xyz, 0.0, d / 1.15)
    assert level == 0 and radius == np.float32(10.0)


def _rotation_case(bins):
    """One keypoint per match on a 30-pixel lattice, match k rotated into histogram bin bins[k] (30 degrees per bin)."""
    p = rs.params(3.0, 64, True)
    pos = [(30.0 + 30.0 * (k % 18), 30.0 + 30.0 * (k // 18)) for k in range(len(bins))]
    cur = rs.frame(p, [(x, y, 0, 0, 0.0, 0) for x, y in pos])
    kf = rs.keyframe([_point(p, x, y, 2.0, angle=30.0 * b) for (x, y), b in zip(pos, bins)])
    tr = {}
    match, nm = rm.search_keyframe_points(p, cur, kf, I4, tr)
    return match, nm, tr


def test_each_branch_of_compute_three_maxima():
    # max2 < 0.1 max1: only the first bin survives
    bins = [0] * 11 + [3]
    match, nm, tr = _rotation_case(bins)
    assert nm == 11 and tr["culled"] == 1 and match.tolist() == list(range(11)) + [-1]
    # max3 < 0.1 max1: two bins survive, the third and a fourth go
    bins = [0] * 21 + [2] * 5 + [4] + [6]
    match, nm, tr = _rotation_case(bins)
    assert nm == 26 and tr["culled"] == 2 and match.tolist() == list(range(26)) + [-1, -1]
    # three bins survive, the fourth goes
    bins = [1] * 5 + [5] * 4 + [7] * 3 + [9]
    match, nm, tr = _rotation_case(bins)
    assert nm == 12 and tr["culled"] == 1 and match.tolist() == list(range(12)) + [-1]
    # a tie for the third place keeps the earlier bin (strict >)
    bins = [1] * 5 + [5] * 4 + [7] * 3 + [9] * 3
    match, nm, tr = _rotation_case(bins)
    assert nm == 12 and tr["culled"] == 3


def test_a_culled_keypoint_stays_taken_during_the_loop():
    """The NULLing happens after the loop: a keypoint whose match is culled was still skipped by the later queries."""
    p = rs.params(3.0, 64, True)
    pos = [(30.0 + 30.0 * k, 30.0) for k in range(12)]
    cur = rs.frame(p, [(x, y, 0, 0, 0.0, 0) for x, y in pos])
    pts = [_point(p, x, y, 2.0, angle=0.0) for x, y in pos[:11]] + [_point(p, pos[11][0], pos[11][1], 2.0, angle=90.0),
                                                                   _point(p, pos[11][0], pos[11][1], 2.1, angle=0.0)]
    match, nm = rm.search_keyframe_points(p, cur, rs.keyframe(pts), I4)
    assert nm == 11 and match[11] == -1


@pytest.mark.parametrize("th,orb_dist", [(10.0, 100), (3.0, 64)])
def test_gpu_scenes_are_not_vacuous(th, orb_dist):
    """Conditions (not measurements) every main pair of the GPU batch meets under both window settings."""
    p = rs.params(th, orb_dist, True)
    cur, kf, T = rs.ragged_batch(p)
    assert [len(c["kps"]) for c in cur] == rs.N_CUR and [len(k["xyz"]) for k in kf] == rs.N_KF
    for f in rs.MAIN:
        tr = {}
        match, nm = rm.search_keyframe_points(p, cur[f], kf[f], T[f], tr)
        assert sum(1 for a, b in zip(tr["pick"], tr["unconstrained"]) if a >= 0 and b >= 0 and a != b) >= 5, f
        assert tr["culled"] >= 1 and tr["behind"] >= 1, f
        assert cur[f]["held"].mean() >= 0.10 and nm >= 30, f
    # the identity-pose pair carries points at depth 0 of both kinds
    z0 = kf[6]["xyz"][:, 2] == 0
    assert (z0 & (kf[6]["xyz"][:, 0] == 0)).sum() >= 1 and (z0 & (kf[6]["xyz"][:, 0] != 0)).sum() >= 1


# ==== the keyframe database and DetectRelocalizationCandidates ====================================================================================
from fractions import Fraction


def _bv(d):
    """A BowVector {word: value} as the model's (words, values)."""
    return [w for w in sorted(d)], [d[w] for w in sorted(d)]


def _db(kfs):
    db = rm.Database()
    for d in kfs:
        db.add(*_bv(d))
    return db


def test_l1_score_is_one_minus_half_the_l1_distance_exactly():
    """On dyadic values every operation is exact: the score equals 1 - 0.5 * ||v - w||_1 in rational arithmetic (both vectors L1-normalised)."""
    rng = np.random.default_rng(5)
    for _ in range(50):
        def vec():
            ws = sorted(rng.choice(12, size=int(rng.integers(1, 7)), replace=False).tolist())
            parts = rng.multinomial(64, np.ones(len(ws)) / len(ws))
            return {w: p / 64.0 for w, p in zip(ws, parts) if p}
        a, b = vec(), vec()
        l1 = sum(abs(Fraction(a.get(w, 0.0)) - Fraction(b.get(w, 0.0))) for w in set(a) | set(b))
        assert Fraction(rm.l1_score(_bv(a), _bv(b))) == 1 - l1 / 2


@pytest.mark.parametrize("scene", rs.DATABASE_SCENES, ids=lambda s: "k%dL%d" % (s["k"], s["L"]))
def test_inverted_file_walk_equals_the_sorted_key_formulation_and_scenes_are_not_vacuous(scene):
    """The literal walk over inverted lists against per-slot intersection + sort by (first shared word, slot), with erased slots; and the
    conditions every query of the GPU scenes meets."""
    args, V, kfs, covis, queries = rs.database_scene(**scene)
    db = rm.Database()
    for w, v in kfs:
        db.add(w, v)
    for s in (3, 17, 18):
        db.erase(s)
    for q in queries:
        want_keys = rm.detect_by_keys(db, q["bow_word"], q["bow_value"], covis)
        cand, words, score = db.detect(q["bow_word"], q["bow_value"], covis)
        assert cand == want_keys
        if scene not in rs.MAIN_DATABASE_SCENES:
            continue
        assert len(cand) >= 3                                                          # retained candidates
        assert ((words > 0) & (score < 0)).sum() >= 1                                  # shares words, not scored
        scored = np.flatnonzero(score >= 0)
        assert any(c not in scored.tolist() or _best_of_other(db, covis, words, c) for c in cand)
        assert _dedup_count(db, covis, words, score) >= 1, "a pBestKF reached twice"
        assert all(words[s] == 0 for s in (3, 17, 18))


def _acc(db, covis, words, s):
    best, bk = db.kfs[s].mRelocScore, s
    for s2 in covis[s][:10]:
        if 0 <= s2 < len(db.kfs) and db.kfs[s2] is not None and words[s2] > 0 and db.kfs[s2].mRelocScore > best:
            best, bk = db.kfs[s2].mRelocScore, s2
    return bk


def _best_of_other(db, covis, words, c):
    """c is the pBestKF of some other scored keyframe."""
    return any(_acc(db, covis, words, s) == c for s in range(len(db.kfs)) if s != c and db.kfs[s] is not None and words[s] > 0)


def _dedup_count(db, covis, words, score):
    best = [_acc(db, covis, words, s) for s in np.flatnonzero(score >= 0)]
    return len(best) - len(set(best))


@pytest.mark.parametrize("maxw,minw", [(4, 3), (5, 4), (6, 4)])
def test_min_common_words_truncates(maxw, minw):
    """minCommonWords = (int)(max * 0.8f): 3.2 -> 3, 4.0 -> 4, 4.8 -> 4; scored iff mnRelocWords > minCommonWords."""
    q = {w: 1.0 / 8 for w in range(8)}
    db = _db([{w: 1.0 / maxw for w in range(maxw)}, {w: 1.0 / minw for w in range(minw)}, {w: 1.0 / (minw + 1) for w in range(minw + 1)}])
    cand, words, score = db.detect(*_bv(q), [[], [], []])
    assert words.tolist() == [maxw, minw, minw + 1]
    assert score[0] >= 0 and score[1] == -1 and score[2] >= 0


def test_a_stale_score_from_the_previous_query_changes_the_result():
    """Keyframe 1 shares a word with the second query but is not scored in it: it contributes the score the first query left."""
    kfs = [{0: 0.25, 1: 0.25, 2: 0.25, 3: 0.25}, {0: 0.25, 10: 0.25, 11: 0.25, 12: 0.25}, {1: 0.25, 2: 0.25, 3: 0.25, 20: 0.25}]
    covis = [[1], [], []]
    q1 = {10: 0.25, 11: 0.25, 12: 0.25, 0: 0.25}             # scores keyframe 1 highly
    q2 = {0: 0.125, 1: 0.375, 2: 0.25, 3: 0.25}               # keyframe 0: 4 words (score 0.875), 2: 3 words (not > 3), 1: 1 word
    fresh = _db(kfs)
    c_fresh, _, s_fresh = fresh.detect(*_bv(q2), covis)
    db = _db(kfs)
    db.detect(*_bv(q1), covis)
    c_stale, words, s_stale = db.detect(*_bv(q2), covis)
    assert words.tolist() == [4, 1, 3] and s_stale[1] == -1 and s_stale.tolist() == s_fresh.tolist()
    assert c_fresh == [0]                                     # a never-scored neighbour reads 0: keyframe 0 stays its own best
    assert s_stale[0] == np.float32(0.875) and c_stale == [1]  # the 1.0 the first query left on keyframe 1 beats keyframe 0's own 0.875

def test_a_best_keyframe_is_emitted_once_though_reached_twice():
    kfs = [{0: 0.5, 1: 0.5}, {0: 0.5, 1: 0.25, 2: 0.25}, {0: 0.25, 1: 0.5, 3: 0.25}]
    covis = [[], [0], [0]]
    cand, words, score = _db(kfs).detect(*_bv({0: 0.5, 1: 0.5}), covis)
    assert score[0] == 1.0 and cand == [0] and (score >= 0).all()     # 0 itself, and the pBestKF of 1 and of 2


def test_all_scores_zero_give_no_candidate():
    """bestAccScore stays 0 and `accScore > 0` fails: words shared, values zero on the keyframe side."""
    cand, words, score = _db([{0: 0.0, 1: 0.0}]).detect(*_bv({0: 0.5, 1: 0.5}), [[]])
    assert words.tolist() == [2] and score[0] == 0.0 and cand == []


def test_erase_then_add_keeps_list_order():
    """The erased keyframe leaves a dead slot; the new one goes to the end of every list, so equal-first-word keyframes keep add order."""
    v = {0: 0.5, 1: 0.5}
    db = _db([v, v, v])
    db.erase(1)
    assert db.add(*_bv(v)) == 3 and db.size() == (4, 3)
    cand, words, score = db.detect(*_bv(v), [[], [], [], []])
    assert cand == [0, 2, 3] and words.tolist() == [2, 0, 2, 2]
    db.clear()
    assert db.size() == (0, 0) and db.add(*_bv(v)) == 0

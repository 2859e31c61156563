"""CPU checks of the plane-association and Manhattan-detection models (tests/plane_match_model.py, tests/manhattan_model.py): the literal
loops equal independent formulations on random box rooms, and hand-built frames pin each quirk of the reference that the device kernels
must reproduce.  No GPU."""
import numpy as np
import pytest

from manhattanslam_amd import plane
from tests import manhattan_model as mm
from tests import plane_match_model as pmm
from tests import plane_scenes as sc

F32 = np.float32
PRM = sc.params()


def _associated(fr):
    n, match, _ = pmm.search_map_by_coefficients(fr, PRM)
    return dict(fr, plane_match=match), n


@pytest.mark.parametrize("block", range(4))
def test_literal_association_equals_prefix_scan(block):
    for seed in range(block * 60, block * 60 + 60):
        fr, _, _ = sc.room(seed, pts=(0, 12))
        a = pmm.search_map_by_coefficients(fr, PRM)
        b = pmm.search_prefix_scan(fr, PRM)
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2].tobytes() == b[2].tobytes(), seed


def test_literal_manhattan_equals_first_maximum():
    hits = partial = 0
    for seed in range(300):
        fr, _ = _associated(sc.room(1000 + seed, pts=(0, 6), n_frame=int(6 + seed % 5))[0])
        found, full, _, cand = mm.detect_manhattan(fr, PRM["mf_ver_th"])
        fm = mm.first_maximum(fr, PRM["mf_ver_th"])
        assert (cand is None) == (fm is None) and (cand is None or cand[:3] == fm[:3] and cand[4] == fm[4]), seed
        hits += found
        partial += found and not full
    assert hits > 100 and 10 < partial < hits                               # both kinds are exercised


_frame = sc.frame


def test_a_match_is_kept_when_a_later_call_finds_nothing():
    fr = _frame([[0, 0, 1, -1]], [[1, 0, 0, 0]], [[[0, 0, 0]]], match=[[5, 7, 9]])
    n, match, _ = pmm.search_map_by_coefficients(fr, PRM)
    assert n == 0 and match.tolist() == [[5, 7, 0]]                          # only the vertical slot is written
    fr = _frame([[0, 0, 1, -1]], [[0.5, 0.5, 0.7071, 0]], [[[0, 0, 0]]], match=[[5, 7, 9]])
    n, match, _ = pmm.search_map_by_coefficients(fr, PRM)
    assert n == 0 and match.tolist() == [[5, 7, 9]]                          # neither test passes: everything kept
    w, h = pmm.pose_layout(match, fr["mp_w"])
    assert h.tolist() == [0] and not w.any()                                  # indices beyond the map's planes are NULL in the pose layout


def test_angle_pass_distance_fail_becomes_the_parallel_plane():
    fr = _frame([[0, 0, 1, -1]], [[0, 0, 1, -3]], [[[0, 0, 3]]])
    n, match, _ = pmm.search_map_by_coefficients(fr, PRM)
    assert n == 0 and match.tolist() == [[-1, 0, -1]]


def test_bad_planes_are_skipped():
    fr = _frame([[0, 0, 1, -1]], [[0, 0, 1, -1], [0, 0, 1, -1]], [[[0, 0, 1]], [[0, 0, 1.05]]], flags=[0, 1])
    n, match, _ = pmm.search_map_by_coefficients(fr, PRM)
    assert n == 1 and match[0, 0] == 1


def test_empty_and_nan_clouds_give_100():
    pM = np.array([0, 0, 1, -1], F32)
    assert pmm.point_distance_from_plane(pM, np.zeros((0, 3))) == 100.0
    assert pmm.point_distance_from_plane(pM, [[np.nan, 0, 0], [0, np.nan, 1]]) == 100.0
    assert pmm.point_distance_from_plane(pM, [[np.nan, 0, 0], [0, 0, 1.5]]) == 0.5
    fr = _frame([[0, 0, 1, -1]], [[0, 0, 1, -1]], [[]])
    fr["mp_clouds"] = [np.zeros((0, 3), F32)]
    assert pmm.search_map_by_coefficients(fr, dict(PRM, d_th=200.0))[1][0, 0] == 0   # 100 < 200: a match at distance 100
    assert pmm.search_map_by_coefficients(fr, PRM)[1][0, 0] == -1


def test_first_wins_on_ties():
    fr = _frame([[0, 0, 1, -1]], [[0, 0, 1, -1]] * 3 + [[1, 0, 0, 0]] * 2, [[[0, 0, 1.1]]] * 3 + [[[0, 0, 0]]] * 2)
    n, match, _ = pmm.search_map_by_coefficients(fr, PRM)
    assert n == 1 and match.tolist() == [[0, 1, 3]]                          # the equal second plane falls through to parallel


_mf_frame, AXES = sc.mf_frame, sc.AXES


def test_a_partial_pair_with_a_larger_score_replaces_a_full_triple():
    fr = _mf_frame(AXES, [10, 10, 10, 500], full=[[0, 1, 2, 0, 0, 1, 2]], part=[[1, 3, 0, 1, 3]])
    found, full, _, cand = mm.detect_manhattan(fr, 0.1)
    assert found == 1 and full == 0 and cand[:3] == (1, 3, -1)
    fr = _mf_frame(AXES, [10, 10, 10, 5], full=[[0, 1, 2, 0, 0, 1, 2]], part=[[1, 3, 0, 1, 3]])
    assert mm.detect_manhattan(fr, 0.1)[1] == 1


def test_first_maximum_wins_ties_and_minus_one_skips():
    fr = _mf_frame(AXES, [10, 10, 10, 10], part=[[0, 1, 0, 0, 1], [0, 2, 0, 0, 2], [1, 2, 0, 1, 2]])
    assert mm.detect_manhattan(fr, 0.1)[3][:3] == (0, 1, -1)
    fr = _mf_frame(AXES, [10, 10, 10, 10], part=[[0, 1, 0, -1, 1], [0, 2, 0, 0, 2]])
    assert mm.detect_manhattan(fr, 0.1)[3][:3] == (0, 2, -1)


def test_determinant_flip_only_in_the_partial_case():
    # partial: c1 x c2 = e3 for (e2, e1) gives det -1 -> flipped to +1
    fr = _mf_frame([[0, 1, 0, -1], [1, 0, 0, -1]], [10, 10], part=[[0, 1, 0, 0, 1]])
    cand = mm.detect_manhattan(fr, 0.1)[3]
    MFc, MFm = mm.frames_of(fr, cand)
    assert mm.det3(MFc) > 0 and mm.det3(MFm) > 0
    # full: a left-handed triple stays left-handed
    fr = _mf_frame([[0, 1, 0, -1], [1, 0, 0, -1], [0, 0, 1, -1]], [10, 10, 10], full=[[0, 1, 2, 0, 0, 1, 2]])
    cand = mm.detect_manhattan(fr, 0.1)[3]
    MFc, _ = mm.frames_of(fr, cand)
    assert cand[2] == 2 and mm.det3(MFc) < 0


def test_not_found_leaves_rcw_untouched():
    fr = _mf_frame(AXES, [10, 10, 10, 10])
    r = np.arange(9, dtype=F32)
    found, full, R, cand = mm.detect_manhattan(fr, 0.1, r)
    assert found == 0 and cand is None and R.tobytes() == r.tobytes()


def test_rotation_of_a_consistent_room_is_the_true_one():
    n = 0
    for seed in range(40):
        fr, R, _ = sc.room(2000 + seed, noise_deg=0.0, n_frame=8)
        fr, _ = _associated(fr)
        found, _, Rcw, _ = mm.detect_manhattan(fr, PRM["mf_ver_th"])
        if found:
            n += 1
            assert np.max(np.abs(Rcw.reshape(3, 3) - R)) < 1e-4, seed
    assert n > 10


def test_pack_sorts_tables():
    full = plane.sort_full([[5, 1, 3, 0, 50, 10, 30], [0, 2, 1, 1, 0, 2, 1]])
    assert full.tolist() == [[0, 1, 2, 1, 0, 1, 2], [1, 3, 5, 0, 10, 30, 50]]
    part = plane.sort_part([[4, 2, 0, 40, 20], [1, 3, 1, 10, 30]])
    assert part.tolist() == [[1, 3, 1, 10, 30], [2, 4, 0, 20, 40]]


# ---- the fast model paths equal the literal ones, and the scenes of tests/test_plane_limits_gpu.py do what they are for -------------------
def _same_association(fr, prm):
    with np.errstate(invalid="ignore"):                                       # the non-finite scenes
        a = pmm.search_map_by_coefficients(fr, prm)
        others = pmm.search_prefix_scan(fr, prm), pmm.search_fast(fr, prm)
    for other in others:
        assert a[0] == other[0] and np.array_equal(a[1], other[1]), (a[0], other[0], a[1], other[1])
        assert np.array_equal(a[2], other[2], equal_nan=True)
    return a


def _same_candidates(fr, caps=None):
    strip = lambda cs: [(c[0], c[1], c[2], c[3].tolist(), c[4], c[5], c[6]) for c in cs]
    a, b = mm.candidates(fr, PRM["mf_ver_th"], caps), mm.candidates_fast(fr, PRM["mf_ver_th"], caps)
    assert strip(a) == strip(b)
    fm, best = mm.first_maximum(fr, PRM["mf_ver_th"], caps), mm.detect_manhattan(fr, PRM["mf_ver_th"], None, caps)[3]
    assert (fm is None) == (best is None) and (fm is None or fm[:3] == best[:3] and fm[4] == best[4])
    return a, best


def test_fast_paths_equal_the_literal_ones_on_random_rooms():
    for seed in range(300):
        fr = sc.room(1000 + seed, pts=(0, 6), n_frame=int(6 + seed % 5))[0]
        a = pmm.search_map_by_coefficients(fr, PRM)
        b = pmm.search_fast(fr, PRM)
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2].tobytes() == b[2].tobytes(), seed
        _same_candidates(dict(fr, plane_match=a[1]))


def test_association_quirk_and_threshold_frames_state_the_models_answers():
    for prm, rows in ((PRM, sc.association_quirks()), (dict(PRM, d_th=0.25), sc.threshold_frames()), (sc.PROBE, sc.nonfinite_frames())):
        for name, fr, match, n in rows:
            got = _same_association(fr, prm)
            assert got[0] == n and got[1].tolist() == match, (name, got[:2])
    fr = {x[0]: x[1] for x in sc.association_quirks()}["empty_cloud"]
    assert _same_association(fr, dict(PRM, d_th=200.0))[1].tolist() == [[0, -1, -1]]
    nan = {x[0]: x[1] for x in sc.nonfinite_frames()}
    assert np.isnan(pmm.search_fast(nan["nan_coef"], sc.PROBE)[2][1:]).all() and np.isnan(pmm.search_fast(nan["inf_tcw"], sc.PROBE)[2][:, 0]).all()


def test_group_frames_match_on_every_lane():
    frames = sc.group_frames()
    assert [len(fr["plane_coef"]) for fr in frames] == [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64]
    got = [pmm.search_fast(fr, PRM) for fr in frames]
    assert got[0][0] == 1 and got[-1][0] == 64 and all(0 < g[0] <= len(fr["plane_coef"]) for g, fr in zip(got, frames))
    assert any(g[0] < len(fr["plane_coef"]) for g, fr in zip(got, frames))
    for fr in sc.group_frames(counts=(1, 5, 17)):
        _same_association(fr, PRM)


def test_probe_frames_end_at_their_targets():
    rows = sc.lane_frames(8, 5) + [sc.stride_frame((0, 1, 63, 65, 129))] + sc.nan_lane_frames(8, 5)
    for fr, targets in rows:
        assert _same_association(fr, sc.PROBE)[1][:, 0].tolist() == targets
    rows = sc.lane_frames() + [sc.stride_frame()] + sc.nan_lane_frames()
    assert {t for _, ts in rows[:4] for t in ts} == set(range(64))           # every lane is some frame plane's target
    for fr, targets in rows:
        assert pmm.search_fast(fr, sc.PROBE)[1][:, 0].tolist() == targets
    # the minimum of a cloud decides: without its one near point the walk ends elsewhere
    fr, targets = sc.lane_frames()[0]
    clouds = list(fr["mp_clouds"])
    clouds[targets[3]] = np.delete(clouds[targets[3]], targets[3], 0)
    assert pmm.search_fast(dict(fr, mp_clouds=clouds), sc.PROBE)[1][3, 0] != targets[3]


def test_csr_clouds_follow_the_documented_rule():
    fr, pts, off = sc.csr_frame()
    clouds = sc.csr_clouds(pts, off, len(pts))
    assert [len(c) for c in clouds] == [12, 0, 16, 11, 9, 0, 0, 6, 17]
    assert clouds[2][0].tobytes() == clouds[0][4].tobytes()                    # overlapping ranges share points
    got = _same_association(dict(fr, mp_clouds=clouds), sc.PROBE)
    assert got[0] == 17 and len(set(got[1][:, 0].tolist())) > 3


def test_big_map_and_huge_cloud_scenes():
    fr, wins = sc.big_map_frame(M=48, K=9)
    got = _same_association(fr, PRM)
    assert got[1][:3, 0].tolist() == wins == [47, 0, 46]
    fr = sc.huge_cloud_frame(P=300, K=17)
    got = _same_association(fr, dict(PRM, d_th=0.5))
    assert got[1][:, 0].tolist() == [-1] + [1] * 16 and got[0] == 16
    assert pmm.search_fast(dict(fr, mp_clouds=[fr["mp_clouds"][0], fr["mp_clouds"][1][:-1]]), dict(PRM, d_th=0.5))[0] == 0   # the last point alone


def test_wide_batches_carry_their_known_frames():
    frames, known = sc.wide_association_batch()
    assert len(frames) == 300 and sorted(known) == [0, 255, 256, 299]
    for f, (match, n) in known.items():
        got = pmm.search_fast(frames[f], PRM)
        assert got[0] == n and got[1].tolist() == match, f
    frames, known = sc.wide_manhattan_batch()
    assert len(frames) == 300 and sorted(known) == [0, 255, 256, 299]
    for f, (found, full, want) in known.items():
        got = mm.detect_manhattan(frames[f], PRM["mf_ver_th"], fast=True)
        assert got[:2] == (found, full) and (got[3] is None if want is None else list(got[3][:3]) == want), f


def test_manhattan_quirk_frames_state_the_models_answers():
    for name, fr, found, full, want in sc.manhattan_quirks():
        cand = _same_candidates(fr)[1]
        got = mm.detect_manhattan(fr, 0.1)
        assert got[:2] == (found, full) and (cand is None if want is None else list(cand[:3]) == want), name


def test_tie_frames_are_decided_by_order():
    for variant, want in ((None, [0, 1, 2]), ("a", [9, 10, 11]), ("b", [10, 11, -1]), ("c", [3, 4, -1]), ("d", [3, 4, 5])):
        fr, w = sc.tie_frame(12, variant)
        assert w == want and len(fr["full"]) <= 64 and len(fr["part"]) <= 64
        assert list(_same_candidates(fr)[1][:3]) == want, variant
    for variant, want in ((None, [0, 1, 2]), ("a", [61, 62, 63]), ("b", [62, 63, -1]), ("c", [3, 4, -1]), ("d", [3, 4, 5])):
        fr, w = sc.tie_frame(64, variant)
        assert w == want
        c = mm.candidates_fast(fr, PRM["mf_ver_th"])
        top = max(x[4] for x in c)
        first = next(x for x in c if x[4] == top)
        assert list(first[:3]) == want and list(mm.detect_manhattan(fr, PRM["mf_ver_th"], fast=True)[3][:3]) == want, variant
        if variant is None:
            assert sum(x[4] == top for x in c) > 1000                         # thousands of candidates share the top score
        else:
            assert sum(x[4] == 60 for x in c) > 1000 and sum(x[4] == top for x in c) == (1 if variant in "ab" else 2)


def test_score_frames_reach_int_max_without_overflow():
    for name, fr, found, want, score in sc.score_frames():
        cands, best = _same_candidates(fr)
        assert (best is None) == (not found) and (best is None or list(best[:3]) == want and best[4] == score), name
        for c in cands:                                                       # the kernel's left-to-right int sums stay in range
            kn = [int(fr["kf_npts"][c[5]][q]) for q in c[6]]
            terms = kn + [int(fr["plane_npts"][p]) for p in c[:3] if p >= 0]
            assert all(abs(sum(terms[:q])) <= sc.INT_MAX for q in range(1, len(terms) + 1)), name
    assert sorted(c[4] for c in mm.candidates(sc.score_frames()[0][1], 0.1)) == [sc.INT_MAX - 1, sc.INT_MAX]
    assert sorted(c[4] for c in mm.candidates(sc.score_frames()[2][1], 0.1)) == [-10, 0, 6]


def test_big_table_scene_finds_its_keys_at_both_ends():
    fr, rows = sc.big_table_frame(fcap=64, qcap=64, mcap=40, kcap=6, pcap=12)
    assert rows["full"][0] == 0 and rows["full"][-1] == 63 and 0 < rows["full"][1] < 63
    assert rows["part"][0] == 0 and rows["part"][-1] == 63 and 0 < rows["part"][1] < 63
    from manhattanslam_amd import plane
    assert np.array_equal(plane.sort_full(fr["full"]), fr["full"]) and np.array_equal(plane.sort_part(fr["part"]), fr["part"])
    cands, best = _same_candidates(fr, (12, 6))
    hit = {tuple(c[3][:3].tolist()) for c in cands if c[2] >= 0} | {tuple(c[3][:2].tolist()) for c in cands if c[2] < 0}
    assert {(0, 1, 2), (9, 10, 11), (37, 38, 39), (0, 1), (9, 10), (38, 39)} <= hit
    assert list(best[:3]) == [9, 10, 11] and best[5] == 5 and sorted(best[6]) == [0, 5, 11]
    assert list(mm.detect_manhattan(dict(fr, full=fr["full"][:0]), 0.1, None, (12, 6))[3][:3]) == [10, 11, -1]
    fr, rows = sc.big_table_frame()                                           # full size: the dictionary path only
    assert (rows["full"][0], rows["full"][-1], rows["part"][0], rows["part"][-1]) == (0, 65535, 0, 65535)
    assert len(fr["full"]) == len(fr["part"]) == 65536 and 20000 < rows["full"][1] < 45000 and 20000 < rows["part"][1] < 45000
    best = mm.detect_manhattan(fr, 0.1, None, (64, 4096), fast=True)[3]
    assert list(best[:3]) == [9, 10, 11] and best[5] == 4095 and sorted(best[6]) == [0, 5, 63]


def test_gate_scene_rejects_what_would_otherwise_win():
    fr, want = sc.gate_frame()
    assert want == [2, 3, -1] and list(_same_candidates(fr)[1][:3]) == want
    best = mm.detect_manhattan(fr, 0.1)[3]
    assert best[4] == 620 and best[6] == [2, 2]                               # the first position's index for both planes ...
    assert np.linalg.matrix_rank(mm.frames_of(fr, best)[1]) == 1              # ... so MFm has rank 1: this winner's Rcw is not defined
    for name in sc.GATES:
        fr, want = sc.gate_frame(name)
        best = _same_candidates(fr)[1]
        assert list(best[:3]) == want and best[4] >= 1000000, name


def test_polar64_agrees_with_the_float_svd_on_well_conditioned_frames():
    worst = 0.0
    kinds = set()
    for fr, kind in sc.polar_frames():
        kinds.add(kind)
        a = mm.detect_manhattan(fr, 0.1)
        b = mm.detect_manhattan(fr, 0.1, polar_fn=mm.polar64)
        assert a[0] == 1 and a[1] == (kind != "partial")
        MFc, MFm = mm.frames_of(fr, a[3])
        lens = np.linalg.norm(MFm[:, :2], axis=0)
        assert lens.min() >= 0.24 and lens.max() <= 4.01 and abs(MFm[:, 0] @ MFm[:, 1]) / (lens[0] * lens[1]) <= 0.51
        assert (mm.det3(MFm) < 0) == (kind == "left")
        R = b[2].reshape(3, 3).astype(np.float64)
        assert np.max(np.abs(R @ R.T - np.eye(3))) < 1e-6                    # a rotation (or a reflection, for a left-handed triple)
        worst = max(worst, float(np.max(np.abs(a[2].astype(np.float64) - b[2]))))
    assert kinds == {"right", "left", "partial"} and worst < 1e-5
    for name, fr, found, _, _ in sc.manhattan_quirks():
        if found:
            assert np.max(np.abs(mm.detect_manhattan(fr, 0.1)[2] - mm.detect_manhattan(fr, 0.1, polar_fn=mm.polar64)[2])) <= 2e-6, name

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


def _frame(coef, mp_w, clouds, flags=None, match=None, Tcw=None):
    coef = np.asarray(coef, F32).reshape(-1, 4)
    return dict(plane_coef=coef, Tcw=np.asarray(Tcw if Tcw is not None else [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F32),
                plane_match=np.full((len(coef), 3), -1, np.int32) if match is None else np.asarray(match, np.int32),
                mp_w=np.asarray(mp_w, F32).reshape(-1, 4), mp_flags=np.ones(len(mp_w), np.uint8) if flags is None else np.asarray(flags, np.uint8),
                mp_clouds=[np.asarray(c, F32).reshape(-1, 3) for c in clouds], plane_npts=np.full(len(coef), 100, np.int32))


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


def _mf_frame(coef, npts, full=(), part=(), kf_npts=None):
    """Frame planes i held by map plane i, one keyframe observing map plane q at index q with the same coefficients."""
    coef = np.asarray(coef, F32).reshape(-1, 4)
    K = len(coef)
    fr = _frame(coef, coef, [[]] * K, match=[[i, -1, -1] for i in range(K)])
    fr.update(plane_npts=np.asarray(npts, np.int32), full=np.asarray(full, np.int32).reshape(-1, 7),
              part=np.asarray(part, np.int32).reshape(-1, 5), kf_Rwc=np.eye(3, dtype=F32).reshape(1, 9), kf_coef=[coef],
              kf_npts=[np.asarray(kf_npts if kf_npts is not None else [10] * K, np.int32)])
    return fr


AXES = [[1, 0, 0, -1], [0, 1, 0, -1], [0, 0, 1, -1], [0, 0, 1, -2]]


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

"""tests/keyframe_model.py against itself and against tests/mappoint_model.py: the closed form of the walk's length equals the literal loop;
one case per pin of msl_points_3d; the KeyFrame-form rows equal msl_refresh_map_points' model on a one-observation table, as bytes; every
condition of NeedNewKeyFrame flipped on its own, with the float and double pins on inputs where the two types disagree.  No GPU."""
import numpy as np
import pytest

from tests import keyframe_model as km
from tests import keyframe_scenes as ks
from tests import mappoint_model as mm

F32 = np.float32
IDENT = np.eye(4, dtype=F32)[:3]


def frame(depth, held=None, octave=3, xy=None, Tcw=IDENT):
    n = len(depth)
    kps = np.zeros(n, ks.keypoint_dtype())
    kps["x"], kps["y"] = (np.linspace(10, 600, n), np.linspace(20, 400, n)) if xy is None else xy
    kps["octave"] = octave
    desc = np.arange(n * 32, dtype=np.int64).reshape(n, 32).astype(np.uint8)
    return dict(kps_un=kps, depth=np.asarray(depth, F32), desc=desc, Tcw=Tcw, cur_held=np.full(n, -1, np.int32) if held is None else np.asarray(held, np.int32))


def run(mode, fr, pt_nobs=None, **prm):
    return km.points_3d(mode, km.params(**prm), fr["kps_un"], fr["depth"], fr["desc"], fr["Tcw"], fr["cur_held"], pt_nobs)


def test_closed_form_equals_the_literal_loop():
    rng = np.random.default_rng(3)
    seen = set()
    for _ in range(3000):
        n = int(rng.integers(0, 301))
        th = F32(rng.choice([1.0, 2.5, 3.0, np.inf]))
        mp = int(rng.choice([0, 1, 5, 100, 299, 400]))
        depth = (rng.integers(-2, 50, n) * 0.125).astype(F32)          # ties, zeros, negatives, and th itself
        kind = rng.random(n)
        depth[kind < 0.04] = np.nan
        depth[(kind >= 0.04) & (kind < 0.08)] = np.inf
        depth[(kind >= 0.08) & (kind < 0.12)] = th
        held = np.where(rng.random(n) < 0.5, rng.integers(0, 40, n), -1).astype(np.int32)
        nobs = rng.integers(0, 3, 40).astype(np.int32)
        fr = frame(depth, held)
        members = [z for z in depth if z > 0]
        want = km.walk_length_closed(members, th, mp)
        order, cleared, walked = km.walk(depth, [int(i) if i >= 0 else None for i in held], nobs, th, mp)
        assert walked == want and len(order) <= want and set(cleared) <= set(order), (n, th, mp)
        seen.add((want == len(members), want > mp + 1))
        if n < 40:                                                     # the same loop inside the whole model
            assert run(km.KEYFRAME, fr, nobs, th_depth=th, min_points=mp)["n_walked"] == want
            assert run(km.ALL, fr)["n_walked"] == len(members)
    assert seen == {(True, False), (True, True), (False, False), (False, True)}   # both ends of the walk, with and beyond min_points


def test_th_depth_itself_is_not_far():
    fr = frame([3.0] * 5 + [3.5] * 5)
    assert run(km.KEYFRAME, fr, th_depth=3.0, min_points=2)["n_walked"] == 6      # the five at th_depth are near: the break is at the first 3.5
    fr = frame([np.nextafter(F32(3.0), F32(4.0))] * 5 + [3.5] * 5)
    assert run(km.KEYFRAME, fr, th_depth=3.0, min_points=2)["n_walked"] == 3


@pytest.mark.parametrize("m,near,walked", [(100, True, 100), (101, True, 101), (102, True, 102), (100, False, 100), (101, False, 101), (102, False, 101)])
def test_exactly_100_101_102_members(m, near, walked):
    got = run(km.KEYFRAME, frame([1.0 if near else 4.0] * m))
    assert got["n_walked"] == walked and got["n_new"] == walked and list(got["new_order"][:walked]) == list(range(walked))


def test_equal_depths_straddling_the_cut_go_by_index():
    depth = [5.0] * 8
    depth[6] = 1.0
    got = run(km.KEYFRAME, frame(depth), min_points=3)                 # sorted: 6, 0, 1, 2 | 3, ...: the walk handles four
    assert got["n_walked"] == 4 and list(got["new_order"][:5]) == [6, 0, 1, 2, -1] and got["pt_new"].tolist() == [1, 1, 1, 0, 0, 0, 1, 0]


def test_held_points_with_and_without_observations():
    nobs = np.array([0, 2], np.int32)
    fr = frame([1.0, 2.0, 2.5, 4.0], held=[0, 1, -1, 0])
    for mode in (km.KEYFRAME, km.FRAME):
        got = run(mode, fr, nobs, min_points=0)
        assert got["pt_new"].tolist() == [1, 0, 1, 1] and got["cleared"].tolist() == [1, 0, 0, 1]   # no observations: cleared and fresh
        assert got["n_walked"] == 4 and got["n_new"] == 3 and got["held_out"].tolist() == [-1, 1, -1, -1]   # the held point counts, creates nothing
    got = km.points_3d(km.KEYFRAME, km.params(min_points=0), fr["kps_un"], fr["depth"], fr["desc"], fr["Tcw"], fr["cur_held"], nobs, first_id=70)
    assert got["held_out"].tolist() == [70, 1, 71, 72]
    assert run(km.ALL, fr, nobs)["cleared"].tolist() == [0, 0, 0, 0] and run(km.ALL, fr, nobs)["pt_new"].tolist() == [1, 1, 1, 1]


def test_min_points_zero():
    assert run(km.KEYFRAME, frame([4.0, 5.0, 6.0]), min_points=0)["n_walked"] == 1     # the first far member ends the walk
    assert run(km.KEYFRAME, frame([1.0, 5.0, 6.0]), min_points=0)["n_walked"] == 2
    assert run(km.KEYFRAME, frame([]), min_points=0)["n_walked"] == 0


def test_an_octave_outside_the_levels():
    for octave in (8, -1):
        fr = frame([1.0, 2.0], octave=np.array([octave, 3]))
        kf, fm = run(km.KEYFRAME, fr), run(km.FRAME, fr)
        assert kf["pt_new"].tolist() == [1, 1] and not kf["new_normal"][0].any() and not kf["new_dist"][0].any() and kf["new_dist"][1].all()
        assert fm["new_normal"][0].any() and not fm["new_dist"][0].any() and kf["new_xyz"].tobytes() == fm["new_xyz"].tobytes()
        assert kf["new_desc"].tobytes() == fr["desc"].tobytes()


def test_a_minus_zero_normal_component_survives_in_the_frame_form_only():
    # cv::gemm's double sum starts at +0, so x3D.x is -0 only by rounding: a denormal entry of mRwc times x3Dc.x is a negative double below
    # the smallest float, which rounds to -0.0f; mOw is +0, so P - Ow = (-0, y, z)
    T = np.array([[-1e-45, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], F32)
    p = km.params()
    fr = frame([2.0], xy=(np.array([p["cx"] + F32(0.5)]), np.array([100.0])), Tcw=T)
    assert T[0, 0] < 0
    kf, fm = run(km.KEYFRAME, fr), run(km.FRAME, fr)
    assert np.signbit(fm["new_normal"][0, 0]) and fm["new_normal"][0, 0] == 0 and not np.signbit(kf["new_normal"][0, 0])
    assert kf["new_normal"][0, 1:].tobytes() == fm["new_normal"][0, 1:].tobytes() and kf["new_dist"].tobytes() == fm["new_dist"].tobytes()


def test_keyframe_form_equals_the_refresh_model_on_a_one_observation_table():
    fr = ks.ragged()[9]                                                # 257 slots of every kind
    prm = ks.point_params()
    got = km.points_3d(km.ALL, prm, fr["kps_un"], fr["depth"], fr["desc"], fr["Tcw"])
    ids = [int(i) for i in got["new_order"][:got["n_new"]]]
    assert len(ids) > 150
    table = [dict(desc=fr["desc"], kps_un=fr["kps_un"], Tcw=fr["Tcw"])]
    points = dict(flags=np.ones(len(ids), np.uint8), xyz=got["new_xyz"][ids], ref=np.zeros(len(ids), np.int32))
    want = mm.refresh_map_points(prm, table, [[(0, i)] for i in ids], points, list(range(len(ids))))
    bad = (want["status"] & mm.BAD_OCTAVE) != 0
    assert bad.any() and not bad.all()
    assert want["out_desc"].tobytes() == got["new_desc"][ids].tobytes()
    assert want["out_normal"].tobytes() == got["new_normal"][ids].tobytes() and want["out_dist"].tobytes() == got["new_dist"][ids].tobytes()


# ---- NeedNewKeyFrame -----------------------------------------------------------------------------------------------------------------------
def decide(n_inl=50, n_ref=60, n_near_map=10, n_near_other=10, n_planes=0, prm=None, **record):
    """A frame with n_inl inlier points (observed), n_near_map of them close, n_near_other close slots without a point, and a reference
    keyframe that tracks n_ref points."""
    n = n_inl + n_near_other
    depth = np.full(n, 5.0, F32)
    depth[:n_near_map] = 1.0
    depth[n_inl:] = 1.0
    held = np.full(n, -1, np.int32)
    held[:n_inl] = 0
    fr = dict(ks.RECORD, ref_kf=0, depth=depth, cur_held=held, outlier=np.zeros(n, np.uint8), cur_lheld=np.zeros(0, np.int32),
              line_outlier=np.zeros(0, np.uint8), plane_match=np.zeros((n_planes, 3), np.int32), plane_outlier=np.zeros((n_planes, 3), np.uint8))
    fr.update(record)
    return km.keyframe_decision(dict(ks.DECISION_PARAMS, **(prm or {})), fr, [np.zeros(n_ref, np.int32)], np.array([5], np.int32), np.array([1], np.uint8),
                                np.zeros(1, np.int32))


BASE = dict(last_keyframe_id=95, local_mapping_idle=0)                  # 5 frames since the keyframe, busy: c1a, c1b off


def test_each_condition_flips_on_its_own():
    # 50 inliers of 60 tracked, ratioMap 0.5: nothing holds
    r = decide(**BASE)
    assert r["cond"] == 0 and r["need_kf"] == 0 and r["track_ok"] == 1 and list(r["counts"]) == [60, 20, 10, 10] and r["n_inliers"] == 50
    assert decide(**dict(BASE, last_keyframe_id=70))["cond"] == km.C1A                                  # 100 >= 70 + 30
    assert decide(**dict(BASE, last_keyframe_id=71))["cond"] == 0
    assert decide(**dict(BASE, local_mapping_idle=1), prm=dict(min_frames=5))["cond"] == km.C1B        # 100 >= 95 + 5, idle
    assert decide(**dict(BASE, local_mapping_idle=1), prm=dict(min_frames=6))["cond"] == 0
    assert decide(n_inl=24, n_ref=100, n_near_map=24, n_near_other=0, **BASE)["cond"] == km.C1C | km.C2   # 24 < 25; c2's 24 < 75 as well
    assert decide(n_inl=50, n_ref=60, **BASE)["cond"] == 0 and decide(n_inl=50, n_ref=67, **BASE)["cond"] == km.C2   # 50 < 67 * 0.75f = 50.25
    assert decide(n_inl=50, n_ref=60, n_near_map=10, n_near_other=19, **BASE)["cond"] == km.C2         # ratioMap 10 / 29 < 0.35, not < 0.3
    assert decide(n_inl=50, n_ref=60, n_near_map=10, n_near_other=24, **BASE)["cond"] == km.C1C | km.C2   # 10 / 34 < 0.3
    r = decide(n_inl=50, n_ref=67, **dict(BASE, last_keyframe_id=70))
    assert r["cond"] == km.C1A | km.C2 and r["need_kf"] == 1
    assert decide(n_inl=15, n_ref=100, n_near_map=15, n_near_other=0, **BASE)["cond"] == km.C1C        # c2 wants more than 15 inliers
    assert decide(n_inl=350, n_ref=100, n_near_map=10, n_near_other=30, **BASE)["cond"] == km.C1C      # 0.25: below 0.3, not below thMapRatio = 0.20


def test_float_and_double_products_where_they_disagree():
    # nRefMatches * thRefRatio is a float product: 0.4f is 0.4000000059..., so 25 * 0.4f rounds to 10.0f and 10 < 10.0f is false; in double
    # 25 * (double)0.4f = 10.00000015 and 10 < it would be true.  c1c off (10 >= 6.25, ratioMap 0.5), c2 wants > 15: scale by 2
    assert F32(50) * F32(0.4) == F32(20.0) and 50 * float(F32(0.4)) > 20.0
    r = decide(n_inl=20, n_ref=50, n_kfs=1, **BASE)
    assert r["cond"] == 0                                              # the float product: 20 < 20.0f is false
    # nRefMatches * 0.25 is a double product and exact; (float)mnMatchesInliers is exact here: the boundary is the integer itself
    assert decide(n_inl=25, n_ref=100, n_near_map=25, n_near_other=0, **BASE)["cond"] & km.C1C == 0
    # ratioMap passes through double: 3 / 10 in double rounds to the float 0.3f exactly, so `< 0.3f` is false
    assert F32(np.float64(F32(3)) / 10.0) == F32(0.3)
    assert decide(n_inl=30, n_ref=30, n_near_map=3, n_near_other=7, **BASE)["cond"] & km.C1C == 0
    # the id sums wrap at 2^32: last_keyframe_id = 2^32 - 10 (as int32: -10) + 30 = 20 <= 100
    assert decide(**dict(BASE, last_keyframe_id=-10))["cond"] == km.C1A and decide(**dict(BASE, last_keyframe_id=-10, frame_id=19))["cond"] == 0


def test_new_plane_overrides_and_the_queue_branch():
    r = decide(n_planes=1, plane_match=np.array([[-1, 2, 2]], np.int32), **BASE)
    assert r["new_plane"] == 1 and r["cond"] == 0 and r["need_kf"] == 1 and r["track_ok"] == 1         # busy, but the queue is short
    assert decide(n_planes=1, plane_match=np.array([[-1, 2, 2]], np.int32), **dict(BASE, keyframes_in_queue=3))["need_kf"] == 0
    assert decide(n_planes=1, plane_match=np.array([[-1, 2, 2]], np.int32), **dict(BASE, keyframes_in_queue=3, local_mapping_idle=1))["need_kf"] == 1
    r = decide(n_planes=1, plane_match=np.array([[-1, 2, 2]], np.int32), plane_outlier=np.array([[1, 1, 0]], np.uint8), **BASE)
    assert r["new_plane"] == 0 and r["plane_match"].tolist() == [[-1, -1, 2]] and r["plane_outlier"].tolist() == [[1, 0, 0]]
    r = decide(n_planes=2, plane_match=np.array([[4, -1, 5], [3, 1, 1]], np.int32), plane_outlier=np.array([[1, 1, 1], [0, 0, 0]], np.uint8), **BASE)
    assert r["plane_match"].tolist() == [[-1, -1, -1], [3, 1, 1]] and r["plane_outlier"].tolist() == [[1, 1, 0], [0, 0, 0]]
    assert r["new_plane"] == 0 and r["n_inliers"] == 51               # the outlier map plane is NULLed with its byte kept: no new plane


def test_only_tracking_and_the_other_early_returns():
    r = decide(n_inl=24, prm=dict(only_tracking=1), **dict(BASE, last_keyframe_id=0))
    assert r["need_kf"] == 0 and r["cond"] == 0 and not r["counts"].any() and r["track_ok"] == 1
    fr = dict(n_inl=24, **dict(BASE, last_keyframe_id=0))
    assert decide(**fr)["need_kf"] == 1 and decide(local_mapping_stopped=1, **fr)["need_kf"] == 0
    assert decide(last_reloc_frame_id=71, n_kfs=31, **fr)["need_kf"] == 0 and decide(last_reloc_frame_id=71, n_kfs=30, **fr)["need_kf"] == 1
    assert decide(last_reloc_frame_id=70, n_kfs=31, **fr)["need_kf"] == 1
    # only_tracking counts a point without observations as an inlier; the clean-up still NULLs it
    zero = dict(n_inl=8, n_near_other=0)
    args = (np.zeros(1, np.int32), np.array([1], np.uint8), np.zeros(1, np.int32))
    fr8 = dict(ks.RECORD, depth=np.ones(8, F32), cur_held=np.zeros(8, np.int32), outlier=np.zeros(8, np.uint8), cur_lheld=np.zeros(0, np.int32),
               line_outlier=np.zeros(0, np.uint8), plane_match=np.zeros((0, 3), np.int32), plane_outlier=np.zeros((0, 3), np.uint8))
    r = km.keyframe_decision(dict(ks.DECISION_PARAMS, only_tracking=1), fr8, [np.zeros(0, np.int32)], *args)
    assert r["n_inliers"] == 8 and r["track_ok"] == 1 and r["found_pt"].all() and (r["held_out"] == -1).all() and zero
    r = km.keyframe_decision(ks.DECISION_PARAMS, fr8, [np.zeros(0, np.int32)], *args)
    assert r["n_inliers"] == 0 and r["track_ok"] == 0 and r["found_pt"].all() and (r["held_out"] == 0).all()   # not ok: not cleaned


def test_track_ok_thresholds_and_a_stale_inlier_count():
    assert decide(n_inl=7, **BASE)["track_ok"] == 1 and decide(n_inl=6, **BASE)["track_ok"] == 0
    assert decide(n_inl=19, **dict(BASE, last_reloc_frame_id=71))["track_ok"] == 0 and decide(n_inl=20, **dict(BASE, last_reloc_frame_id=71))["track_ok"] == 1
    assert decide(n_inl=19, **dict(BASE, last_reloc_frame_id=70))["track_ok"] == 1
    # TrackLocalMap did not run: the member keeps its value, however many points the frame holds
    r = decide(n_inl=50, n_ref=100, flags=km.TRACK_OK, n_inliers_in=24, **BASE)
    assert r["n_inliers"] == 24 and r["cond"] == km.C1C | km.C2 and r["need_kf"] == 1 and not r["found_pt"].any()
    assert decide(n_inl=50, flags=0, n_inliers_in=24, **BASE)["track_ok"] == 0
    assert decide(n_inl=50, flags=km.TRACK_OK | km.NEW_PLANE, n_inliers_in=50, **BASE)["need_kf"] == 1
    assert decide(n_inl=50, flags=km.TRACKED_LOCAL_MAP | km.NEW_PLANE, **BASE)["need_kf"] == 0     # SearchMapByCoefficients reset the member


def test_the_fixed_scenes_reach_every_branch():
    res = ks.decision_model()
    assert {r["track_ok"] for r in res} == {0, 1} and {r["need_kf"] for r in res} == {0, 1} and {r["new_plane"] for r in res} == {0, 1}
    conds = {int(r["cond"]) for r in res}
    assert any(c & km.C1A for c in conds) and any(c & km.C1B for c in conds) and any(c & km.C1C for c in conds) and any(c & km.C2 for c in conds)
    for mode in (km.ALL, km.KEYFRAME, km.FRAME):
        m = ks.point_model("ragged", mode, 4097)
        assert m["n_new"][0] == 0 and m["n_new"][-1] > 100 and (mode == km.ALL or (m["n_walked"] > m["n_new"]).any())
        assert mode == km.ALL or (m["cleared"].any() and (m["n_walked"][-1] < (ks.ragged()[-1]["depth"] > 0).sum()))

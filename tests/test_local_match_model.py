"""First-principles checks of the CPU model of Tracking::SearchLocalPoints (tests/local_match_model.py), each against a hand-computed
answer.  No GPU.  Camera: identity pose, fx = fy = 512, principal point (320, 240), 640 x 480, so a point (X, Y, 2) projects to
(320 + 256 X, 240 + 256 Y) exactly and lies at distance 2 from the optical centre when X = Y = 0."""
import numpy as np

from tests import local_match_model as lm
from tests import local_match_scenes as ls

F32 = np.float32
T = np.eye(4, dtype=np.float32)
Z = (0.0, 0.0, 1.0)             # normal along the viewing ray of (0, 0, 2): viewCos = 1


def P(th=3.0):
    return ls.params(th, fx=512.0, fy=512.0, cx=320.0, cy=240.0)


def run(kps, pts, th=3.0):
    p = P(th)
    return lm.search_local_points(p, ls.frame(p, kps), ls.points(pts), T)


def test_behind_the_camera_is_not_in_view():
    _, ntm, nm, inv, _ = run([(320, 240, 0, 0, -1, 0)], [((0, 0, -2), Z, (1, 3), 3)])
    assert ntm == 0 and nm == 0 and inv[0] == 0


def test_projection_on_the_image_bound_is_in_view():
    # X = 1.25 -> u = 512 * 1.25 * 0.5 + 320 = 640 = mnMaxX exactly: "u > mnMaxX" is false, the point is in view; X = 1.2501 -> u = 640.0256
    _, ntm, _, inv, trk = run([], [((1.25, 0, 2), Z, (1, 3), 3), ((1.2501, 0, 2), Z, (1, 3), 3)])
    assert list(inv) == [1, 0] and ntm == 1
    assert trk["proj_x"][0] == F32(640) and trk["proj_y"][0] == F32(240) and trk["proj_xr"][0] == F32(620)   # u - 40 * 0.5


def test_distance_just_outside_the_invariance_range():
    # dist = 2 exactly.  In: 1.2f * dmax >= 2 and 0.8f * dmin <= 2.  Out: the neighbouring floats.
    dmax = F32(2) / F32(1.2)
    while F32(1.2) * dmax < F32(2):
        dmax = np.nextafter(dmax, F32(3))
    dmax_out = np.nextafter(dmax, F32(0))
    dmin = F32(2) / F32(0.8)
    while F32(0.8) * dmin > F32(2):
        dmin = np.nextafter(dmin, F32(0))
    dmin_out = np.nextafter(dmin, F32(3))
    assert F32(1.2) * dmax_out < F32(2) and F32(0.8) * dmin_out > F32(2)
    pts = [((0, 0, 2), Z, (1, dmax), 1), ((0, 0, 2), Z, (1, dmax_out), 1), ((0, 0, 2), Z, (dmin, 3), 1), ((0, 0, 2), Z, (dmin_out, 3), 1)]
    _, ntm, _, inv, _ = run([], pts)
    assert list(inv) == [1, 0, 1, 0] and ntm == 2


def test_view_cos_just_below_the_limit():
    # PO = (0, 0, 2), |PO| = 2: viewCos = (2 * nz) / 2 = nz exactly
    below = np.nextafter(F32(0.5), F32(0))
    _, ntm, _, inv, trk = run([], [((0, 0, 2), (0, 0, below), (1, 3), 1), ((0, 0, 2), (0, 0, 0.5), (1, 3), 1)])
    assert list(inv) == [0, 1] and trk["view_cos"][1] == F32(0.5)


def test_radius_by_viewing_cos_around_0998():
    # float(0.998) = 0.99800002... > 0.998 (double): radius 2.5 * th; the float just below is < 0.998: radius 4 * th.  At level 0 (mfMaxDistance
    # = dist: log(1) = 0) the scale factor is 1, so with th = 3 the window half-width is 7.5 or 12 px; a keypoint 10 px away tells them apart.
    hi, lo = F32(0.998), np.nextafter(F32(0.998), F32(0))
    assert float(hi) > 0.998 > float(lo)
    kps = [(330, 240, 0, 5, -1, 0)]
    m_hi, _, nm_hi, _, t_hi = run(kps, [((0, 0, 2), (0, 0, hi), (1, 2), 1)])
    m_lo, _, nm_lo, _, t_lo = run(kps, [((0, 0, 2), (0, 0, lo), (1, 2), 1)])
    assert t_hi["scale_level"][0] == 0 and t_lo["scale_level"][0] == 0
    assert nm_hi == 0 and m_hi[0] == -1
    assert nm_lo == 1 and m_lo[0] == 0


def test_predicted_level_zero_admits_only_octave_zero():
    # mfMaxDistance = dist: level ceil(log(1) / log 1.2) = 0; GetFeaturesInArea(.., -1, 0) keeps octave 0 only
    pt = [((0, 0, 2), Z, (1, 2), 1)]
    m, _, nm, _, trk = run([(321, 240, 1, 0, -1, 0), (322, 240, 0, 30, -1, 0)], pt)
    assert trk["scale_level"][0] == 0 and nm == 1 and list(m) == [-1, 0]
    # level 1 (mfMaxDistance = 2.2: ceil(0.52) = 1) admits octaves 0 and 1: the closer descriptor at octave 1 wins
    m, _, nm, _, trk = run([(321, 240, 1, 0, -1, 0), (322, 240, 0, 30, -1, 0)], [((0, 0, 2), Z, (1, 2.2), 1)])
    assert trk["scale_level"][0] == 1 and nm == 1 and list(m) == [0, -1]


def test_ratio_test_same_level_rejects_across_levels_accepts():
    # best 10, second 12: 10 > 0.8 * 12 = 9.6
    pt = [((0, 0, 2), Z, (1, 2.2), 1)]                 # level 1: octaves 0 and 1 pass
    m, _, nm, _, _ = run([(321, 240, 1, 10, -1, 0), (322, 240, 1, 12, -1, 0)], pt)
    assert nm == 0 and list(m) == [-1, -1]
    m, _, nm, _, _ = run([(321, 240, 1, 10, -1, 0), (322, 240, 0, 12, -1, 0)], pt)
    assert nm == 1 and list(m) == [0, -1]
    # best 9 <= 9.6 at the same level: accepted
    m, _, nm, _, _ = run([(321, 240, 1, 9, -1, 0), (322, 240, 1, 12, -1, 0)], pt)
    assert nm == 1 and list(m) == [0, -1]


def test_preheld_keypoints():
    # keypoint 0 held on entry by a point with observations: skipped, the point takes keypoint 1; held without observations: overwritten
    pt = [((0, 0, 2), Z, (1, 2), 1)]
    m, _, nm, _, _ = run([(321, 240, 0, 0, -1, 3), (322, 240, 0, 40, -1, 0)], pt)
    assert nm == 1 and list(m) == [-1, 0]
    m, _, nm, _, _ = run([(321, 240, 0, 0, -1, 1), (322, 240, 0, 40, -1, 0)], pt)
    assert nm == 1 and list(m) == [0, -1]


def test_stereo_check_on_track_proj_xr():
    # proj_xr = 320 - 40 / 2 = 300; window half-width 7.5: uright 307 passes, 308 does not
    pt = [((0, 0, 2), Z, (1, 2), 1)]
    m, _, nm, _, _ = run([(321, 240, 0, 0, 308, 0), (322, 240, 0, 50, 307, 0)], pt)
    assert nm == 1 and list(m) == [-1, 0]


def test_order_of_the_local_points_decides():
    # two points whose best keypoint is keypoint 0 (distance 0); keypoint 1 (distance 60, other octave: no ratio test) is the second choice.
    # A has observations, B not.  A then B: A takes 0 and B must skip it -> B takes 1.  B then A: B takes 0, A overwrites it; nothing holds 1.
    kps = [(321, 240, 0, 0, -1, 0), (322, 240, 1, 60, -1, 0)]
    A = ((0, 0, 2), Z, (1, 2.2), 3)
    B = ((0, 0, 2), Z, (1, 2.2), 1)
    m, ntm, nm, _, _ = run(kps, [A, B])
    assert ntm == 2 and nm == 2 and list(m) == [0, 1]
    m, ntm, nm, _, _ = run(kps, [B, A])
    assert ntm == 2 and nm == 2 and list(m) == [1, -1]


def test_not_a_candidate_is_not_projected():
    _, ntm, nm, inv, trk = run([(320, 240, 0, 0, -1, 0)], [((0, 0, 2), Z, (1, 2), 2)])
    assert ntm == 0 and nm == 0 and inv[0] == 0 and trk["scale_level"][0] == 0 and trk["proj_x"][0] == 0


def test_random_scene_is_mostly_matched():
    """Sanity of the scene generator the GPU tests use: many points in view, many matches, no keypoint pre-held with observations handed out."""
    p = ls.params(3.0)
    cur, local, Tcw = ls.random_frame(7, p, n_cur=300, n_local=600)
    m, ntm, nm, inv, trk = lm.search_local_points(p, cur, local, Tcw)
    assert 300 < ntm < 600 and nm > 80 and inv.sum() == ntm
    assert len(np.unique(trk["scale_level"][inv == 1])) >= 4
    assert not np.any((cur["flags"] == 3) & (m >= 0))

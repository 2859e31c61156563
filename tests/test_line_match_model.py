"""First-principles checks of the sequential line-matching model (tests/line_match_model.py): hand-computed cases for each quirk of
GetLinesInArea, isInFrustum(MapLine*), PredictScale, RadiusByViewingCos and the greedy hand-out that DESIGN.md section 3 pins.  CPU only."""
import math

import numpy as np

from tests import line_match_model as lmm
from tests import line_match_scenes as lsc

F32 = np.float32


def _kl(rows):
    """rows: (x, y, angle, octave)."""
    from manhattanslam_amd import KEYLINE_DTYPE
    kl = np.zeros(len(rows), KEYLINE_DTYPE)
    for i, r in enumerate(rows):
        kl[i] = r
    return kl


def test_slope_test_has_no_fabs():
    """(y1 - y2) / (x1 - x2) - angle > r * 0.01 rejects; a negative difference always passes (src/Frame.cc:401-403)."""
    kl = _kl([(5, 0, 10.0, 0), (5, 0, -10.0, 0), (5, 0, -0.14, 0), (5, 0, -0.16, 0)])
    # a horizontal segment (slope 0) from (0, 0) to (10, 0), midpoint (5, 0), r = 15: r * 0.01 = 0.15
    assert lmm.get_lines_in_area(kl, 0, 0, 10, 0, 15) == [0, 2]


def test_vertical_segment_slopes():
    """x1 == x2: (y1 - y2) / 0 is -inf (passes) or +inf (rejected); a point segment gives NaN, which passes."""
    kl = _kl([(5, 5, 0.0, 0)])
    assert lmm.get_lines_in_area(kl, 5, 0, 5, 10, 15) == [0]         # (0 - 10) / 0 = -inf
    assert lmm.get_lines_in_area(kl, 5, 10, 5, 0, 15) == []          # (10 - 0) / 0 = +inf
    assert lmm.get_lines_in_area(kl, 5, 5, 5, 5, 15) == [0]          # 0 / 0 = NaN


def test_distance_is_compared_with_the_float_r_squared():
    """The squared midpoint distance (double, rounded to float) against r * r in float: equality passes."""
    kl = _kl([(3, 4, 0.0, 0)])
    assert lmm.get_lines_in_area(kl, -1, 0, 1, 0, 5.0) == [0]        # 25 > 25 is false
    assert lmm.get_lines_in_area(kl, -1, 0, 1, 0, np.nextafter(F32(5), F32(0))) == []
    # the midpoint is 0.5 * (x1 + x2) of the FLOAT sum: 2^24 + 1 rounds to 2^24 before the halving
    kl = _kl([(2.0 ** 23 + 1, 0, 0.0, 0)])
    assert lmm.get_lines_in_area(kl, 2.0 ** 24, 0, 1, 0, 0.6) == []   # midpoint 8388608, 1 away (the exact 8388608.5 would pass)
    assert lmm.get_lines_in_area(kl, 2.0 ** 24, 0, 1, 0, 1.2) == [0]


def test_levels_are_checked_only_for_positive_bounds():
    """bCheckLevels = minLevel > 0 || maxLevel > 0 (src/Frame.cc:391); maxLevel < 0 = no upper bound."""
    kl = _kl([(0, 0, 0.0, o) for o in range(8)])
    seg = (-1, 0, 1, 0, 5)
    assert lmm.get_lines_in_area(kl, *seg, -1, 0) == list(range(8))   # local search, predicted level 0: no level check
    assert lmm.get_lines_in_area(kl, *seg, 0, 1) == [0, 1]           # level 1: octaves 0 .. 1
    assert lmm.get_lines_in_area(kl, *seg, 0) == list(range(8))      # forward window at nLastOctave 0: unchecked
    assert lmm.get_lines_in_area(kl, *seg, 2) == list(range(2, 8))   # forward at 2: no upper bound
    assert lmm.get_lines_in_area(kl, *seg, 0, 0) == list(range(8))   # backward at 0: unchecked
    assert lmm.get_lines_in_area(kl, *seg, 0, 2) == [0, 1, 2]
    assert lmm.get_lines_in_area(kl, *seg, -1, 1) == [0, 1]          # both ways at 0: checked (maxLevel 1 > 0)
    assert lmm.get_lines_in_area(kl, *seg, lmm.wrap(lmm.INT_MIN - 1), lmm.INT_MIN) == []   # a level of INT_MIN: L - 1 wraps to INT_MAX


def test_radius_by_viewing_cos_at_the_boundary():
    """viewCos > 0.998 compares a float with a double: the float nearest 0.998 is above it and gets the 5-pixel radius."""
    assert float(F32(0.998)) > 0.998
    assert lmm.radius_by_viewing_cos(F32(0.998)) == 5.0
    assert lmm.radius_by_viewing_cos(np.nextafter(F32(0.998), F32(0))) == 8.0
    assert lmm.radius_by_viewing_cos(F32(1.0)) == 5.0


def test_predict_scale_is_not_clamped():
    """MapLine::PredictScale has no clamp: -1 at the near end of the window, nlevels and nlevels + 1 past the far end, INT_MIN at distance 0."""
    ls_ = F32(math.log(1.2))
    assert lmm.predict_level(F32(1.0), F32(1.2), ls_) == -1         # ratio 1 / 1.2
    assert lmm.predict_level(F32(1.2 ** 7.5), F32(1.0), ls_) == 8
    assert lmm.predict_level(F32(1.2 ** 8.5), F32(1.0), ls_) == 9
    assert lmm.predict_level(F32(2.0), F32(0.0), ls_) == lmm.INT_MIN
    assert [lmm.clamp_level(v, 8) for v in (-1, 0, 7, 8, 9, lmm.INT_MIN)] == [0, 0, 7, 7, 7, 0]


def _frame(p, kl_rows, dists):
    """A current frame: keylines and descriptors at the given Hamming distances from the all-zero descriptor."""
    from tests.local_match_scenes import desc_at
    return dict(kl=_kl(kl_rows), desc=np.stack([desc_at(d) for d in dists]), ends=np.zeros((len(kl_rows), 4)),
                flags=np.zeros(len(kl_rows), np.uint8))


def _line_at(p, u1, v1, u2, v2, z=2.0):
    """The world segment (identity pose) whose endpoints project to (u1, v1) and (u2, v2) at depth z."""
    fx, fy, cx, cy = (float(p[k][0]) for k in ("fx", "fy", "cx", "cy"))
    return [(u1 - cx) / fx * z, (v1 - cy) / fy * z, z, (u2 - cx) / fx * z, (v2 - cy) / fy * z, z]


def _last(p, lines, flags, octaves):
    m = len(lines)
    return dict(xyz=np.array(lines, np.float64).reshape(m, 6), desc=np.zeros((m, 32), np.uint8), flags=np.array(flags, np.uint8),
                octave=np.array(octaves, np.int32))


def test_ratio_test_only_on_one_level():
    """Best 10 / second 12: rejected on one octave (10 > 0.6 * 12), accepted across octaves."""
    p = lsc.params(15.0)
    T = np.eye(4, dtype=np.float32)
    seg = _line_at(p, 300, 200, 340, 200)
    last = _last(p, [seg], [1], [0])
    same = _frame(p, [(320, 200, 0.0, 0), (321, 200, 0.0, 0)], [10, 12])
    diff = _frame(p, [(320, 200, 0.0, 0), (321, 200, 0.0, 1)], [10, 12])
    assert lmm.search_lines_by_projection(p, same, last, T, T)[1] == 0
    m, n = lmm.search_lines_by_projection(p, diff, last, T, T)
    assert n == 1 and list(m) == [0, -1]


def test_later_line_overwrites_and_counts():
    """Two lines without observations pick one keyline: the later one holds it and both count (nmatches 2)."""
    p = lsc.params(15.0)
    T = np.eye(4, dtype=np.float32)
    seg = _line_at(p, 300, 200, 340, 200)
    cur = _frame(p, [(320, 200, 0.0, 0)], [5])
    m, n = lmm.search_lines_by_projection(p, cur, _last(p, [seg, seg], [1, 1], [0, 0]), T, T)
    assert n == 2 and list(m) == [1]


def test_holder_with_observations_is_skipped():
    """The first line has observations: the second skips its keyline and takes the next candidate."""
    p = lsc.params(15.0)
    T = np.eye(4, dtype=np.float32)
    seg = _line_at(p, 300, 200, 340, 200)
    cur = _frame(p, [(320, 200, 0.0, 0), (322, 200, 0.0, 1)], [5, 30])
    m, n = lmm.search_lines_by_projection(p, cur, _last(p, [seg, seg], [3, 1], [0, 0]), T, T)
    assert n == 2 and list(m) == [0, 1]
    # local search: a keyline pre-held with observations (flags 3) is never handed out; one held without (flags 1) is overwritten
    pl = lsc.params(1.0)
    cur["flags"] = np.array([3, 1], np.uint8)
    local = dict(xyz=np.array([seg], np.float64), normal=np.array([[0, 0, 1.0]]), dist=np.array([[0.5, 2.5]], np.float32),
                 desc=np.zeros((1, 32), np.uint8), flags=np.array([3], np.uint8))
    m, ntm, n, inv, trk = lmm.search_local_lines(pl, cur, local, T)
    assert ntm == 1 and n == 1 and list(m) == [-1, 0] and inv[0] == 1


def test_local_radius_level_and_track():
    """Local search on a hand-made line: the track record, the 8-pixel radius times th (th 1 has no factor), the unclamped level."""
    pl = lsc.params(1.0)
    T = np.eye(4, dtype=np.float32)
    seg = _line_at(pl, 300, 200, 340, 200)
    local = dict(xyz=np.array([seg], np.float64), normal=np.array([[0.6, 0, 0.8]]), dist=np.array([[0.5, 2.5]], np.float32),
                 desc=np.zeros((1, 32), np.uint8), flags=np.array([1], np.uint8))
    res = lmm.is_in_frustum(pl, T[:3], seg, local["normal"][0], 0.5, 2.5, 0.6, pl["log_scale_factor"])
    u1, v1, u2, v2, level, vc = res
    assert abs(u1 - 300) < 1e-3 and abs(u2 - 340) < 1e-3 and float(vc) < 0.998
    assert level == lmm.predict_level(F32(2.5), F32(math.sqrt(sum(float(x) ** 2 for x in (np.array(seg[:3], F32) * F32(0.5) + np.array(seg[3:], F32) * F32(0.5))))),
                                      pl["log_scale_factor"])
    r8 = F32(8.0) * F32(pl["scale_factors"][0][lmm.clamp_level(level, 8)])
    far = _frame(pl, [(320 + float(r8) + 0.5, 200, 0.0, level)], [0])   # just outside the radius: no match at th 1 ...
    assert lmm.search_local_lines(pl, far, local, T)[2] == 0
    p5 = lsc.params(5.0)                                             # ... inside it at th 5
    assert lmm.search_local_lines(p5, far, local, T)[2] == 1
    # a line behind the camera (one endpoint at Z < 0) is not in view
    back = dict(local, xyz=np.array([seg[:5] + [-2.0]], np.float64))
    assert lmm.search_local_lines(pl, far, back, T)[1] == 0


def test_pose_layout():
    """Written slots carry the writer's world position bit for bit; the last-frame search clears the others, the local one leaves them."""
    xyz = np.arange(12, dtype=np.float64).reshape(2, 6) + 0.1
    init_x, init_h = np.full((3, 6), 7.0), np.array([1, 1, 1], np.uint8)
    lx, lh = lmm.pose_layout(np.array([1, -1]), xyz, 3, init_x, init_h, clear=True)
    assert lx[0].tobytes() == xyz[1].tobytes() and list(lh) == [1, 0, 1] and np.all(lx[1:] == 7.0)
    lx, lh = lmm.pose_layout(np.array([-1, 0]), xyz, 3, init_x, init_h, clear=False)
    assert lx[1].tobytes() == xyz[0].tobytes() and list(lh) == [1, 1, 1] and np.all(lx[0] == 7.0)


def test_scenes_reach_the_quirks():
    """The GPU scenes contain what they claim: levels -1 / 8 / 9 in view, vertical segments, both search modes, matches and conflicts."""
    p = lsc.params(15.0)
    cur, last, Tc, Tl = lsc.frame_pair(504, p, vertical=12)
    pr = [lmm.project_line(p, Tc[:3], last["xyz"][i]) for i in range(12)]
    assert sum(1 for q in pr if q is not None and q[0] == q[2]) >= 3
    modes = {lmm.search_mode(p, t[:3], tl[:3]) for t, tl in (lsc.frame_pair(s, p, fwd=f)[2:] for s, f in ((505, 0.5), (506, -0.5), (507, 0.0)))}
    assert modes == {0, 1, 2}
    pl = lsc.params(1.0)
    cur, local, T = lsc.local_frame(604, pl, n_local=800)
    _, ntm, nm, inv, trk = lmm.search_local_lines(pl, cur, local, T)
    assert {-1, 8, 9} <= set(trk["scale_level"][inv == 1].tolist()) and nm > 0 and ntm > 400

"""CPU checks of the TranslationOptimization model (tests/translation_model.py) on hand-checkable cases: convergence to the true translation,
the rotation left as given, the points-only < 3 exit, a negative n_good, the stale line error, the < 10 edges exit and the untouched
parallel / vertical plane flags."""
import math

import numpy as np
import pytest

from tests import pose_model as pm
from tests import pose_scenes as ps
from tests import translation_model as tm
from tests import translation_scenes as ts


def test_noiseless_scene_converges_to_the_true_translation():
    """Points, lines and planes, every measurement exact at (Rcw, t_true) (set through the model's own error functions), initial translation
    off by about 5 cm: the estimate lands on t_true within 1e-9 and the rotation is the quaternion of Rcw."""
    c = ps.params()
    fr, rcw, R, t = ts.scene(21, max_rot_deg=0.3, n_pts=300, n_lines=12, n_planes=3, noise=0.0, null_frac=0.0, margin=None, c=c)
    Tf = tm.effective_tcw(fr["Tcw"], rcw)
    edges, n0 = tm.build_edges(fr, c, Tf)
    edges += tm.build_plane_edges(fr, c, Tf)
    assert n0 == 300 and {e.kind for e in edges} == {pm.MONO, pm.STEREO, pm.LINE, pm.PLANE}
    T0 = pm.to_se3(Tf)
    Tt = (T0[0], tuple(t))
    for e in edges:
        if e.kind in (pm.MONO, pm.STEREO):
            e.obs = tuple(o - r for o, r in zip(e.obs, tm.compute_error(e, Tt, c)))
        elif e.kind == pm.LINE:
            e.obs = (e.obs[0], e.obs[1], e.obs[2] - tm.compute_error(e, Tt, c)[0])
        else:
            e.obs = tm.plane_add(Tt, e.X)
    assert np.max(np.abs(np.array(T0[1]) - t)) > 0.01
    with tm.translation_edges():
        T = pm.optimize(edges, T0, c, 10)
        for e in edges:                                                       # the Huber weights slow the last digits: one more optimize()
            e.robust = False
        T = pm.optimize(edges, T, c, 10)
    assert np.max(np.abs(np.array(T[1]) - t)) < 1e-9
    assert np.max(np.abs(np.array(T[0]) - np.array(T0[0]))) < 1e-15            # exp(0 rotation) * q, renormalised


def test_output_rotation_is_the_input_rotation():
    c = ps.params()
    for seed in (31, 32):
        fr, rcw, _, _ = ts.scene(seed, n_pts=400, n_lines=10, n_planes=3, c=c)
        n, T, _ = tm.translation_optimization(fr, c, rcw)
        assert n > 200
        assert np.max(np.abs(T.reshape(3, 4)[:, :3] - rcw.reshape(3, 3))) <= 2e-7      # float rounding of the quaternion round trip
        assert np.max(np.abs(T.reshape(3, 4)[:, 3] - fr["Tcw"].reshape(3, 4)[:, 3])) > 1e-3   # the translation moved


def test_lines_and_planes_do_not_count_as_correspondences():
    """2 points, 10 lines, 3 planes: nInitialCorrespondences counts points only, so the call returns 0 with the pose as given apart from
    Rcw; the point and line flags are cleared, the plane flags untouched (no plane edge exists yet)."""
    c = ps.params()
    fr, rcw, _, _ = ts.scene(41, n_pts=2, n_lines=10, n_planes=3, null_frac=0.0, margin=None, c=c)
    fr["line_has"][:] = 1
    fr["plane_outlier"][:] = (1, 0, 1)
    n, T, out = tm.translation_optimization(fr, c, rcw)
    assert n == 0
    want = fr["Tcw"].reshape(3, 4).copy()
    want[:, :3] = rcw.reshape(3, 3)
    assert T.tobytes() == want.reshape(12).tobytes()
    assert not out["outlier"].any() and not out["line_outlier"].any()
    for k in ("plane_outlier", "par_outlier", "ver_outlier"):
        assert np.array_equal(out[k], fr[k])
    assert pm.pose_optimization(fr, c)[0] > 0                                 # PoseOptimization counts lines and planes


def test_bad_planes_make_n_good_negative():
    """3 exact points and 5 planes whose measured normals are 30 degrees off (angle error independent of the translation): every plane is bad,
    nBad = 5 and the return value is 3 - 5 = -2.  8 edges: one round."""
    c = ps.params(angleInfo=2000.0)
    fr, rcw, R, _ = ts.scene(51, max_rot_deg=0.0, n_pts=3, n_lines=0, n_planes=5, noise=0.0, null_frac=0.0, margin=None, c=c)
    for i in range(5):
        n = fr["plane_coef"][i][:3].astype(np.float64)
        fr["plane_coef"][i][:3] = (ps.rot(np.cross(n, [0.3, 0.5, 0.7]), 30.0) @ n).astype(np.float32)
    n, _, out = tm.translation_optimization(fr, c, rcw)
    assert out["plane_outlier"].tolist() == [1] * 5 and not out["outlier"].any()
    assert n == -2


def test_active_line_is_judged_on_its_stale_error():
    """classify() on a hand-made line pair: left active (flag 0) it keeps the error the last trial left (inside 2 * 5.991) although it is far
    off at the estimate; flagged it is re-evaluated there and is bad.  Neither case counts in nBad."""
    c = ps.params()
    T = ((0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0))
    obs = (0.0, 1.0, -c["cy"] - 10.0)                                          # v - cy - 10 = 0: the line y = 10 px below the centre
    edges = [pm.Edge(pm.LINE, 0, obs, (0.0, 0.0, 2.0), (1.0, 1.0, 1.0), pm.DELTA_STEREO),
             pm.Edge(pm.LINE, 0, obs, (0.5, 0.0, 2.0), (1.0, 1.0, 1.0), pm.DELTA_STEREO)]
    assert tm.compute_error(edges[0], T, c)[0] == pytest.approx(-10.0)        # chiline 100 > 11.98 at the estimate
    for flag, want in ((0, 0), (1, 1)):
        for e in edges:
            e.err = (1.0, 0.0, 0.0)                                           # the last trial's error: chiline 1
        out = {"line_outlier": np.array([flag], np.uint8)}
        rows = []
        assert tm.classify(edges, out, T, c, rows) == 0
        assert out["line_outlier"][0] == want, flag
        assert rows[0][2] == (np.float32(1.0) if flag == 0 else np.float32(100.0))


def test_fewer_than_ten_edges_stop_after_one_round(monkeypatch):
    """Points + 2 * lines + planes decides: 5 points + 1 line + 2 planes (9 edges) run one round, 6 points + 1 line + 2 planes (10) all four."""
    c = ps.params()
    calls = []
    real = pm.optimize
    monkeypatch.setattr(pm, "optimize", lambda *a, **k: calls.append(1) or real(*a, **k))
    for n_pts, rounds in ((5, 1), (6, 4)):
        fr, rcw, _, _ = ts.scene(61, n_pts=n_pts, n_lines=1, n_planes=2, null_frac=0.0, par=False, ver=False, margin=None, c=c)
        fr["line_has"][:] = 1
        calls.clear()
        tm.translation_optimization(fr, c, rcw)
        assert len(calls) == rounds, (n_pts, len(calls))


def test_parallel_and_vertical_plane_flags_are_never_touched():
    c = ps.params()
    fr, rcw, _, _ = ts.scene(71, n_pts=200, n_lines=5, n_planes=6, c=c)
    fr["par_outlier"][:] = (1, 0, 1, 1, 0, 0)
    fr["ver_outlier"][:] = (0, 1, 1, 0, 1, 0)
    fr["plane_outlier"][:] = 1
    n, _, out = tm.translation_optimization(fr, c, rcw)
    assert n > 0 and np.array_equal(out["par_outlier"], fr["par_outlier"]) and np.array_equal(out["ver_outlier"], fr["ver_outlier"])
    assert not out["plane_outlier"].all()                                     # the mvpMapPlanes flags were re-classified


def test_model_restores_pose_model_edges():
    """translation_edges() is scoped: PoseOptimization's model is unchanged after (and during a failure inside) a translation call."""
    before = pm.compute_error, pm.jacobian
    with pytest.raises(RuntimeError):
        with tm.translation_edges():
            raise RuntimeError
    assert (pm.compute_error, pm.jacobian) == before
    assert math.isfinite(ps.params()["planeChi"])


def test_point_edges_follow_the_octave_and_reference_rules():
    """The point edges obey msl.h's rules as in pose_model: octaves -1 / 99 give exactly the result of 0 / nlevels - 1, and pt_ref values
    xcap, INT_MAX, -2 and INT_MIN exactly the result of -1 (no edge, not counted, outlier byte kept)."""
    c = ps.params()
    fr, rcw, _, _ = ts.scene(33, n_pts=100, n_lines=3, n_planes=2, margin=None, c=c)
    ok = np.flatnonzero(fr["pt_ref"] >= 0)
    want = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in fr.items()}
    want["octave"][ok[::6]], want["octave"][ok[1::6]] = 0, 7
    fr["octave"][ok[::6]], fr["octave"][ok[1::6]] = -1, 99
    slots = ok[[3, 10, 22, 45]]
    want["pt_ref"][slots] = -1
    fr["pt_ref"][slots] = [len(fr["xyz"]), 2 ** 31 - 1, -2, -2 ** 31]
    fr["outlier"][slots] = want["outlier"][slots] = [1, 1, 0, 1]
    a, b = tm.translation_optimization(fr, c, rcw), tm.translation_optimization(want, c, rcw)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    for k in a[2]:
        assert np.array_equal(a[2][k], b[2][k]), k
    assert list(a[2]["outlier"][slots]) == [1, 1, 0, 1]
    assert tm.build_edges(fr, c, tm.effective_tcw(fr["Tcw"], rcw))[1] == len(ok) - 4

"""CPU checks of the PoseOptimization model (tests/pose_model.py) against independent facts: convergence on a noiseless scene, outlier
flagging, the Huber weight, the LDLT solve, the analytic Jacobians, the SE3 exponential, the < 3 correspondences exit and the stale-chi2
rule of the classification."""
import math

import numpy as np
import pytest

from tests import pose_model as pm
from tests import pose_scenes as ps


def test_noiseless_scene_converges_to_the_true_pose():
    """All six edge kinds, every measurement exact at the true pose (set through the model's own error functions), initial pose off by
    about 2 degrees and 5 cm: the estimate lands on the true pose within 1e-9."""
    c = ps.params()
    fr, R, t = ps.scene(11, n_pts=300, n_lines=12, n_planes=3, noise=0.0, rot_deg=2.0, trans=0.05, null_frac=0.0, margin=None, c=c)
    edges, n0 = pm.build_edges(fr, c)
    assert {e.kind for e in edges} == {pm.MONO, pm.STEREO, pm.LINE, pm.PLANE, pm.PAR, pm.VER}
    Tt = pm.se3_from_Rt(R.tolist(), tuple(t))
    for e in edges:
        if e.kind in (pm.MONO, pm.STEREO):
            err = pm.compute_error(e, Tt, c)
            e.obs = tuple(o - r for o, r in zip(e.obs, err))
        elif e.kind == pm.LINE:
            e.obs = (e.obs[0], e.obs[1], e.obs[2] - pm.compute_error(e, Tt, c)[0])
        elif e.kind in (pm.PLANE, pm.PAR):
            e.obs = pm.plane_transform(Tt, e.X)
        elif e.kind == pm.VER:
            P = pm.plane_transform(Tt, e.X)
            v = pm.cross(P[:3], e.obs[:3])
            vn = math.sqrt(sum(x * x for x in v))
            b = pm.matvec(pm.angle_axis_matrix(math.pi / 2, tuple(x / vn for x in v)), P[:3])
            e.obs = (b[0], b[1], b[2], e.obs[3])
    T0 = pm.to_se3(fr["Tcw"])
    assert np.max(np.abs(np.array(pm.quat_to_matrix(T0[0])) - R)) > 0.01
    T = pm.optimize(edges, T0, c, 10)
    for e in edges:                                                               # the Huber weights slow the last digits: one more optimize()
        e.robust = False
    T = pm.optimize(edges, T, c, 10)
    assert np.max(np.abs(np.array(pm.quat_to_matrix(T[0])) - R)) < 1e-9 and np.max(np.abs(np.array(T[1]) - t)) < 1e-9


def test_gross_outliers_are_flagged_and_counted():
    c = ps.params()
    fr, _, _ = ps.scene(13, n_pts=400, n_lines=0, n_planes=0, outliers=0.0, null_frac=0.0, c=c)
    n_clean, _, out_clean = pm.pose_optimization(fr, c)
    bad = np.arange(0, 400, 10)
    fr["un_xy"][bad] += np.float32(80.0)
    n, T, out = pm.pose_optimization(fr, c)
    assert out["outlier"][bad].all()
    assert n == 400 - int(out["outlier"].sum()) and n <= n_clean - len(bad) + 2


def test_huber_weight_is_one_inside_delta():
    d = pm.DELTA_MONO
    for e2 in (0.0, 1e-3, 1.0, d * d * 0.999, d * d):
        assert pm.robustify(e2, d) == (e2, 1.0)
    r0, r1 = pm.robustify(4 * d * d, d)
    assert r1 == pytest.approx(0.5) and r0 == pytest.approx(3 * d * d)


def test_ldlt_matches_numpy_solve():
    rng = np.random.default_rng(3)
    for _ in range(50):
        A = rng.normal(size=(6, 6))
        H = A @ A.T + np.eye(6) * rng.uniform(0.5, 6)
        b = rng.normal(size=6)
        ok, x = pm.ldlt_solve(H.tolist(), b.tolist())
        assert ok
        ref = np.linalg.solve(H, b)
        assert np.max(np.abs(np.array(x) - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref)))
    ok, x = pm.ldlt_solve(np.diag([1.0, -1, 1, 1, 1, 1]).tolist(), [1.0] * 6)
    assert not ok                                                                # a negative pivot: not positive
    ok, x = pm.ldlt_solve(np.zeros((6, 6)).tolist(), [1.0] * 6)
    assert ok and x == [0.0] * 6                                                 # zero matrix: pseudo-inverse


@pytest.mark.parametrize("kind", [pm.MONO, pm.STEREO, pm.LINE])
def test_analytic_jacobians_match_central_differences(kind):
    c = ps.params()
    rng = np.random.default_rng(4)
    T = pm.se3_exp([0.1, -0.2, 0.05, 0.3, -0.1, 0.2])
    for _ in range(20):
        X = tuple(rng.normal(size=3) + np.array([0, 0, 4.0]))
        obs = (300.0, 200.0, 280.0) if kind != pm.LINE else tuple(np.array([0.6, 0.8, -350.0]))
        e = pm.Edge(kind, 0, obs, X, (1.0, 1.0, 1.0), 1.0)
        J = pm.jacobian(e, T, c)
        h = 1e-3 if kind == pm.STEREO else 1e-6                                # (stereo: cam_project's float invz quantises the error)
        for d in range(6):
            u = [0.0] * 6
            u[d] = h
            ep = pm.compute_error(e, pm.oplus(T, u), c)
            u[d] = -h
            em = pm.compute_error(e, pm.oplus(T, u), c)
            for i in range(len(J)):
                num = (ep[i] - em[i]) / (2 * h)
                tol = (2e-2 if kind == pm.STEREO else 1e-4) * max(1.0, abs(num))
                assert abs(J[i][d] - num) <= tol, (kind, i, d, J[i][d], num)


def test_se3_exp_composed_with_its_inverse_is_identity():
    rng = np.random.default_rng(5)
    for _ in range(20):
        u = list(rng.normal(size=6) * 0.5)
        T = pm.se3_exp(u)
        I = pm.se3_mul(T, pm.se3_inverse(T))
        assert max(abs(v) for v in I[0][:3]) < 1e-15 and abs(I[0][3] - 1) < 1e-15 and max(abs(v) for v in I[1]) < 1e-14
    assert pm.se3_exp([0.0] * 6) == ((0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0))


def test_fewer_than_three_correspondences_returns_zero_pose_unchanged():
    c = ps.params()
    fr, _, _ = ps.scene(14, n_pts=4, n_lines=0, n_planes=0, null_frac=0.0, margin=None, c=c)
    fr["pt_ref"][2:] = -1
    fr["outlier"][:] = 1
    n, T, out = pm.pose_optimization(fr, c)
    assert n == 0 and T.tobytes() == fr["Tcw"].tobytes()
    assert list(out["outlier"]) == [0, 0, 1, 1]                                 # flags of created edges reset, the rest kept


def test_stale_chi2_of_a_rejected_last_trial():
    """optimize() leaves an active edge's error at the last trial it evaluated, even when that trial was rejected and the vertex popped:
    the classification then reads an error that differs from the one at the returned estimate."""
    c = ps.params()
    found = False
    for seed in range(40, 60):
        fr, _, _ = ps.scene(seed, n_pts=60, n_lines=3, n_planes=0, margin=None, c=c)
        edges, _ = pm.build_edges(fr, c)
        T0 = pm.to_se3(fr["Tcw"])
        T = pm.optimize(edges, T0, c, 10)
        stale = [e.err for e in edges]
        fresh = [pm.compute_error(e, T, c) for e in edges]
        if stale != fresh:
            found = True
            break
    assert found, "no scene with a rejected last trial"
    # the model classifies with the stale values: flipping to fresh errors changes at least one chi2
    assert any(pm.chi2(type("E", (), {"err": s, "info": e.info})) != pm.chi2(type("E", (), {"err": f, "info": e.info}))
               for s, f, e in zip(stale, fresh, edges))


def _same_result(a, b):
    assert a[0] == b[0] and np.array_equal(a[1], b[1]), (a[0], b[0])
    for k in a[2]:
        assert np.array_equal(a[2][k], b[2][k]), k


def test_out_of_range_octaves_are_clamped():
    """msl.h: octaves outside [0, nlevels) are clamped.  Octave -1 weighs like octave 0 and octave 99 like nlevels - 1, for every outcome
    (pose, n_good and flags), on an 8-level and a 3-level table."""
    for nlevels in (8, 3):
        c = ps.params(nlevels=nlevels)
        fr, _, _ = ps.scene(31, n_pts=120, n_lines=4, n_planes=2, outliers=0.1, margin=None, c=c, nlevels=nlevels)
        ok = np.flatnonzero(fr["pt_ref"] >= 0)
        lo, hi = ok[::7], ok[3::7]
        clean = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in fr.items()}
        clean["octave"][lo], clean["octave"][hi] = 0, nlevels - 1
        fr["octave"][lo], fr["octave"][hi] = -1, 99
        _same_result(pm.pose_optimization(fr, c), pm.pose_optimization(clean, c))
        edges, _ = pm.build_edges(fr, c)
        w = {e.idx: e.info[0] for e in edges if e.kind in (pm.MONO, pm.STEREO)}
        assert all(w[i] == c["inv_level_sigma2"][0] for i in lo) and all(w[i] == c["inv_level_sigma2"][-1] for i in hi)


def test_out_of_range_point_references_are_null():
    """msl.h: pt_ref values outside [0, xcap) count as NULL: no edge, no correspondence, the outlier byte kept.  xcap, INT_MAX, -2 and
    INT_MIN give exactly the result of -1 in those slots; with an explicit xcap smaller than len(xyz), references at and above it are NULL."""
    c = ps.params()
    fr, _, _ = ps.scene(32, n_pts=100, n_lines=3, n_planes=2, margin=None, c=c)
    ok = np.flatnonzero(fr["pt_ref"] >= 0)
    slots = ok[[2, 9, 17, 40]]
    null = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in fr.items()}
    null["pt_ref"][slots] = -1
    fr["pt_ref"][slots] = [len(fr["xyz"]), 2 ** 31 - 1, -2, -2 ** 31]
    fr["outlier"][slots] = [1, 0, 1, 1]
    null["outlier"][slots] = [1, 0, 1, 1]
    got, want = pm.pose_optimization(fr, c), pm.pose_optimization(null, c)
    _same_result(got, want)
    assert list(got[2]["outlier"][slots]) == [1, 0, 1, 1]
    assert pm.build_edges(fr, c)[1] == pm.build_edges(null, c)[1] == len(ok) - 4 + 3 + 3 * 2
    xcap = 60                                                                     # references >= 60 are NULL under this xcap
    cut = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in null.items()}
    cut["pt_ref"][cut["pt_ref"] >= xcap] = -1
    _same_result(pm.pose_optimization(null, c, xcap=xcap), pm.pose_optimization(cut, c))

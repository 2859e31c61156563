"""The sequential model of msl_pnp_ransac (tests/pnp_model.py) against the true pose, against LAPACK, against the literal loop of
PnPsolver::iterate, and the margins of the fixed scenes (tests/pnp_scenes.py).  CPU only."""
import numpy as np
import pytest

from tests import pnp_model as pm
from tests import pnp_scenes as ps

K = (ps.FX, ps.FY, ps.CX, ps.CY)
# compute_pose on exact data, n = 6 .. 63 generic points: the largest error of an entry of R or t over the twenty sets below, measured with
# this model on the CPU, is 1.02e-7 against the true pose and 8.4e-8 against the LAPACK variant.  The bound is the larger one times 10.
MEASURED_WORST = 1.02e-7
BOUND = 10 * MEASURED_WORST


def _exact(seed):
    sc = ps.pnp_scene(seed, N=6 + seed * 3, sigma_px=0.0, outlier_share=0.0, n_null=0, kcap=200)
    Pw = sc["xyz"][sc["match"]].astype(np.float64)
    T = sc["Tcw_true"].astype(np.float64)
    Pc = Pw @ T[:, :3].T + T[:, 3]
    uv = np.stack([ps.FX * Pc[:, 0] / Pc[:, 2] + ps.CX, ps.FY * Pc[:, 1] / Pc[:, 2] + ps.CY], 1)
    return Pw, uv, T


@pytest.fixture(scope="module")
def exact_runs():
    runs = []
    for seed in range(20):
        Pw, uv, T = _exact(seed)
        runs.append((T, pm.compute_pose(Pw[None], uv[None], K), pm.compute_pose(Pw[None], uv[None], K, eig=pm.lapack_eig)))
    return runs


def test_refine_against_the_true_pose(exact_runs):
    worst = max(max(np.abs(r[0][0] - T[:, :3]).max(), np.abs(r[1][0] - T[:, 3]).max()) for T, r, _ in exact_runs)
    print("worst error against the true pose", worst)
    assert worst <= BOUND


def test_refine_against_lapack(exact_runs):
    worst = max(max(np.abs(r[0][0] - l[0][0]).max(), np.abs(r[1][0] - l[1][0]).max()) for _, r, l in exact_runs)
    print("worst difference from the LAPACK variant", worst)
    assert worst <= BOUND


def test_jacobi_is_an_eigendecomposition():
    rng = np.random.default_rng(5)
    for n in (3, 4, 5, 12):
        B = rng.normal(size=(7, n + 2, n)); A = np.swapaxes(B, 1, 2) @ B
        d, ut = pm.jacobi_eig(A)
        assert np.all(np.diff(d, axis=1) <= 0) and np.allclose(d, np.linalg.eigvalsh(A)[:, ::-1], rtol=1e-12, atol=1e-12 * d.max())
        assert np.allclose(ut @ np.swapaxes(ut, 1, 2), np.eye(n), atol=1e-13)
        assert np.allclose(np.swapaxes(ut, 1, 2) @ (d[:, :, None] * ut), A, atol=1e-12 * d.max())
    assert [len(s) for s in pm.schedule(12)] == [6] * 11 and sorted(p for s in pm.schedule(12) for p in s) == [(a, b) for a in range(12) for b in range(a + 1, 12)]
    assert sorted(p for s in pm.schedule(5) for p in s) == [(a, b) for a in range(5) for b in range(a + 1, 5)]


@pytest.mark.parametrize("name", ["exact", "eleven", "ragged150", "track_b"])
def test_records_against_the_literal_loop(name):
    """Refine() at records only = Refine() at every qualifying iteration, as PnPsolver.cc:199-224 does."""
    sc, p = ps.scene(name)
    a = ps.model(name)
    b = pm.pnp_ransac(p, sc["octave"], sc["un_xy"], sc["match"], sc["xyz"], sc["seed"], literal=True)
    assert b["refines"] >= a["refines"]
    for k in ("status", "n_inliers", "first_success"):
        assert a[k] == b[k], k
    assert np.array_equal(a["inlier"], b["inlier"]) and np.array_equal(a["pt_ref"], b["pt_ref"]) and a["Tcw"].tobytes() == b["Tcw"].tobytes()


@pytest.mark.parametrize("name", list(ps.SCENES))
def test_margins(name):
    """No inlier comparison of a scene comes within 2^-19 (16 float32 ulps) of its threshold: equal flags are a fair demand on the device."""
    m = ps.model(name)
    print(name, "margin", m["margin"], "status", m["status"], "inliers", m["n_inliers"])
    assert m["margin"] >= 2.0 ** -19


def test_scene_outcomes():
    """The scenes exercise what they are meant to."""
    want = dict(empty=0, below=0, exact=2, eleven=1, ragged150=1, track_a=1, track_b=1, no_inliers=0, full=1)
    assert {n: ps.model(n)["status"] for n in want} == want
    r = ps.model("ragged150")
    sc, _ = ps.scene("ragged150")
    assert r["n_inliers"] >= 75 and set(np.nonzero(r["inlier"])[0]) <= set(sc["true_inlier"])
    assert ps.model("full")["n_inliers"] > 7000                         # Refine() over thousands of correspondences
    assert np.abs(r["Tcw"] - sc["Tcw_true"]).max() < 5e-3
    assert ps.model("track_b")["first_success"] > 0                     # an earlier record's Refine() failed or none qualified


def test_edge_rules():
    p = ps.params_dict()
    t = lambda N, **kw: pm.ransac_table(N, kw.get("prob", 0.99), 10, kw.get("max_its", 40), 4, kw.get("eps", 0.5))
    assert t(0) == (10, 1) and t(3) == (10, 1) and t(9) == (10, 1)
    assert t(10) == (10, 1)                                             # N == minInliers: one nominal iteration
    assert t(11) == (10, 4)                                             # epsilon raised to 10 / 11
    assert t(120) == (60, 35) and t(120, max_its=300) == (60, 35) and t(120, max_its=20) == (60, 20)
    assert t(1000, eps=0.05) == (50, 40)
    # the || of PnPsolver.cc:174: maxIts adjusted to 1 still runs n_iterations
    m = ps.model("exact")
    assert (m["N"], m["min_inliers"], m["K"]) == (10, 10, 5) and len(m["count"]) == 5
    assert ps.model("below")["K"] == 0 and ps.model("below")["status"] == 0 and not ps.model("below")["inlier"].any()
    sc, _ = ps.scene("eleven")
    one = pm.pnp_ransac(dict(p, n_iterations=0), sc["octave"], sc["un_xy"], sc["match"], sc["xyz"], sc["seed"])
    assert one["K"] == 4


def test_sampler():
    s = pm.sample_sets(7, 50, 6)
    assert s.shape == (50, 4) and all(len(set(r)) == 4 for r in s.tolist()) and s.min() == 0 and s.max() == 5
    assert np.array_equal(s, pm.sample_sets(7, 50, 6)) and not np.array_equal(s, pm.sample_sets(8, 50, 6))
    assert sorted(pm.sample_sets(3, 1, 4)[0].tolist()) == [0, 1, 2, 3]
    assert int(pm.hash32(0, 0, 0)) == int(pm._fmix(pm._fmix(np.uint64(0)) ^ np.uint64(0x85EBCA77)))

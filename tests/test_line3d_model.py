"""The sequential model of msl_lines_3d (tests/line3d_model.py) on its own: one case per pin, the pinned Jacobi solver against LAPACK on the
quantities the pins make solver-independent, known answers, the margins that make "identical on the device" a fair demand, and the three
selection modes against a literal transcription of the three reference loops.  No GPU."""
import math

import numpy as np
import pytest

from tests import line3d_model as lm
from tests import line3d_scenes as ls
from tests.pnp_model import hash32, jacobi_eig, lapack_eig

# Measured on the scenes (printed by test_jacobi_against_lapack): the largest relative difference of a Mahalanobis
# distance (of those above 1e-6: a sample on the line itself has no relative error) between DU from the pinned solver and from
# numpy.linalg.eigh is 1.2e-13, the largest difference of a refit direction from numpy.linalg.svd's, up to sign, 1.1e-14.  The assertions
# allow ten times that.
DIST_REL_MEASURED, DIR_ABS_MEASURED = 1.2e-13, 1.1e-14


def _lines(name, order=lm.ALL):
    return [(j, r) for j, r in enumerate(ls.model(name, order)["lines"]) if r is not None]


# ---- pins ---------------------------------------------------------------------------------------------------------------------------------
def test_pin_svd_is_the_jacobi_solver():
    """Both cv::SVD uses are jacobi_eig on a symmetric 3x3: cov0 for a sample, P^T P for the refit.  The distance does not depend on the order
    or the signs of DU's rows (to rounding); the sign of d only swaps the end points."""
    r = _lines("refit")[0][1]
    pos, DU = r["pos"], r["DU"]
    d, ut = jacobi_eig(lm.cov0_of(pos, np.float32(ls.PARAMS["fx"])))
    assert np.array_equal((1.0 / np.sqrt(d))[:, :, None] * ut, DU)
    q1, q2 = tuple(pos[0]), tuple(pos[-1])
    base = lm.mah_dist(pos, DU, q1, q2)
    other = lm.mah_dist(pos, DU[:, [2, 0, 1], :] * np.array([1.0, -1.0, 1.0])[None, :, None], q1, q2)
    ok = np.isfinite(base) & (base > 0)
    assert np.max(np.abs(other[ok] - base[ok]) / base[ok]) < 1e-9
    t = r["trace"]
    assert t["refits"] >= 2                                              # the last round was turned down: m, d are the round's before it
    tm, G, _ = t["gram"][-2]
    assert tuple(float(v) for v in jacobi_eig(G)[1][0]) == t["d"] and tm == t["m"]
    pts = [tuple(p) for p in pos]
    i1, i2 = lm._extremes(pts, r["inliers"], t["m"], t["d"])
    j1, j2 = lm._extremes(pts, r["inliers"], t["m"], tuple(-v for v in t["d"]))
    assert (i1, i2) == (j2, j1) and (r["inliers"][i1], r["inliers"][i2]) == t["ends"]


def test_pin_sampler():
    """rand() % left: draw j of iteration k from the keyline's seed with the hash of msl_pnp_ransac, mulhi32(hash, left); one seed per keyline."""
    s = ls.scene("refit")
    for j, r in _lines("refit"):
        n, idx = r["n_kept"], None
        idx = list(range(n))
        for k, (ia, ib, _, _) in enumerate(r["trace"]["iters"]):
            r0 = (int(hash32(int(s["seed"][j]), k, 0)) * n) >> 32
            idx[0], idx[r0] = idx[r0], idx[0]
            r1 = (int(hash32(int(s["seed"][j]), k, 1)) * (n - 1)) >> 32
            idx[1], idx[1 + r1] = idx[1 + r1], idx[1]
            assert (ia, ib) == (idx[0], idx[1])                          # the permutation is carried across the iterations
    a = lm.obtain_3d_line(s["line_ends"][2], s["depth"], s["Tcw"], 1, ls.PARAMS)
    b = lm.obtain_3d_line(s["line_ends"][2], s["depth"], s["Tcw"], 2, ls.PARAMS)
    assert [x[:2] for x in a["trace"]["iters"]] != [x[:2] for x in b["trace"]["iters"]]


def test_pin_null_return_is_line_ok():
    """A failed keyline: line_ok 0 and six zeros; a returned line: line_ok 1 and float-valued world end points."""
    m = ls.model("cells")
    assert m["line_ok"].tolist() == [0, 1] and not m["line_xyz"][0].any() and m["line_xyz"][1].any()
    assert np.array_equal(m["line_xyz"][1], m["line_xyz"][1].astype(np.float32).astype(np.float64))
    assert m["n_support"].tolist() == [0, 39] and m["n_new"] == 1


def test_pin_degenerate_length_and_too_few_samples():
    """numSmp == 0 divides by zero in the reference: no line.  Fewer than min_points samples: no line, and RANSAC is not reached."""
    lines = dict(_lines("short"))
    assert [int(lines[j]["len"]) for j in range(4)] == [0, 8, 9, 10]
    assert [lines[j]["n_kept"] for j in range(4)] == [0, 9, 10, 11]
    assert [lines[j]["ok"] for j in range(4)] == [0, 0, 1, 1] and not lines[0]["trace"]["iters"] and not lines[1]["trace"]["iters"]
    holes = dict(_lines("holes"))
    assert [holes[j]["n_kept"] for j in range(2)] == [9, 10] and [holes[j]["ok"] for j in range(2)] == [0, 1]
    assert not holes[0]["trace"]["iters"] and holes[1]["trace"]["iters"]


def test_pin_get_line_depth_outside_the_image():
    """An end point whose truncated coordinates fall outside the image has depth -1.0f; -0.7 truncates to 0 and is inside."""
    s, m = ls.scene("outside"), ls.model("outside")
    d = s["depth"]
    assert m["line_depth"][0].tolist() == [d[30, 0], d[50, 60]] and m["line_depth"][1, 0] == d[0, 20]
    assert m["line_depth"][3].tolist() == [d[60, 100], -1.0] and m["line_depth"][4].tolist() == [d[100, 30], -1.0]
    assert m["line_depth"][5].tolist() == [-1.0, d[50, 40]]
    assert [r is not None for r in m["lines"]] == [True, True, True, False, False, False, True]
    assert lm.end_depth(d, np.float32(np.nan), 3.0) == -1.0 and lm.end_depth(d, 3.0, np.float32(np.inf)) == -1.0
    assert m["lines"][0]["n_kept"] < int(m["lines"][0]["len"]) + 1                      # the samples with pt.x < 0 are dropped


def test_pin_non_finite_values_propagate():
    """sigma(z) == 0 makes an eigenvalue of cov0 zero: the inverse square root is infinite, the distance NaN, and NaN is not an inlier."""
    z = 0.3453787
    a = z / 100.0
    cov = np.array([np.diag([a * a, a * a, 0.0]), np.diag([a * a, a * a, 1e-4])])
    with np.errstate(all="ignore"):
        DU = lm.du_of(cov)
    assert not np.isfinite(DU[0]).all() and np.isfinite(DU[1]).all()
    pos = np.array([[0.01, 0.002, z], [0.01, 0.002, z]])
    margins = dict(dist=math.inf, cell=math.inf)
    dist = lm.mah_dist(pos, DU, (0.0, 0.0, z), (0.1, 0.0, z))
    assert np.isnan(dist[0]) and np.isfinite(dist[1])
    assert lm._inliers(pos, DU, (0.0, 0.0, z), (0.1, 0.0, z), 1.5, margins) == [1]
    # the scene with depths next to the root still decides every keyline
    assert [r["ok"] for _, r in _lines("sigma_zero")] == [1, 1]


# ---- independent arithmetic ---------------------------------------------------------------------------------------------------------------
def test_jacobi_against_lapack():
    """DU from numpy.linalg.eigh and the refit direction from numpy.linalg.svd: the Mahalanobis distance of every sample and the direction up
    to sign are solver-independent."""
    worst_d = worst_v = 0.0
    for name in ls.ALL_SCENES:
        fx = np.float32(ls.params(name)["fx"])
        for _, r in _lines(name):
            if r["DU"] is None:
                continue
            pos = r["pos"]
            with np.errstate(all="ignore"):
                DU2 = lm.du_of(lm.cov0_of(pos, fx), lapack_eig)
            for q1, q2 in ((tuple(pos[0]), tuple(pos[-1])), (tuple(pos[len(pos) // 2]), tuple(pos[1]))):
                a, b = lm.mah_dist(pos, r["DU"], q1, q2), lm.mah_dist(pos, DU2, q1, q2)
                ok = np.isfinite(a) & np.isfinite(b) & (a > 1e-6)
                assert np.array_equal(np.isfinite(a), np.isfinite(b))
                if ok.any():
                    worst_d = max(worst_d, float(np.max(np.abs(a[ok] - b[ok]) / a[ok])))
            for tm, G, idx in r["trace"]["gram"]:
                v = jacobi_eig(G)[1][0]
                w = np.linalg.svd(pos[idx] - np.array(tm))[2][0]
                worst_v = max(worst_v, float(min(np.max(np.abs(v - w)), np.max(np.abs(v + w)))))
    print("largest relative distance difference", worst_d, "largest direction difference", worst_v)
    assert worst_d <= 10 * DIST_REL_MEASURED and worst_v <= 10 * DIR_ABS_MEASURED


# ---- known answers ------------------------------------------------------------------------------------------------------------------------
def test_noiseless_plane_returns_first_and_last_sample():
    for name, j in (("one", 0), ("wave", 0), ("wave", 1), ("wave", 2), ("big", 0), ("integer", 0)):
        r = ls.model(name)["lines"][j]
        assert r["ok"] == 1 and sorted(r["trace"]["ends"]) == [0, r["n_kept"] - 1] and r["n_support"] == r["n_kept"], (name, j)
    assert [r["n_kept"] for _, r in _lines("wave")] == [63, 64, 65]
    assert [r["n_kept"] for _, r in _lines("big")][:4] == [101] * 4


def test_depth_step_returns_the_longer_side():
    s = ls.scene("step")
    for j, r in _lines("step"):
        _, pix = lm.sample_pixels(s["line_ends"][j], s["depth"].shape, ls.PARAMS)
        far = np.array([c >= 64 for _, c in pix])
        assert len(pix) == r["n_kept"] and r["ok"] == 1
        side = far if far.sum() > (~far).sum() else ~far
        assert side[r["inliers"]].all() and len(r["inliers"]) >= 0.9 * side.sum(), (j, r["inliers"])
        assert side[list(r["trace"]["ends"])].all()


def test_scenes_reach_what_they_are_for():
    cells = dict(_lines("cells"))
    assert cells[0]["n_kept"] >= 10 and all(rec == 0 for *_, rec in cells[0]["trace"]["iters"]) and len(cells[0]["trace"]["iters"]) == 10
    acc = dict(_lines("accept"))
    assert [acc[j]["ok"] for j in range(4)] == [0, 1, 0, 1] and all(acc[j]["n_support"] >= 10 for j in range(4))
    assert acc[0]["n_support"] / acc[0]["len"] < 0.4 < acc[1]["n_support"] / acc[1]["len"]
    assert max(r["trace"]["refits"] for _, r in _lines("refit")) >= 3
    assert any(c == -1 or rec == 0 for _, r in _lines("refit") for _, _, c, rec in r["trace"]["iters"])
    full = ls.model("full", lm.DEPTH_ORDER)
    assert int(full["line_ok"].sum()) > 31 and full["n_new"] < int(full["line_ok"].sum())
    assert ls.model("none")["n_new"] == 0 and len(ls.model("none")["line_ok"]) == 0 and len(ls.model("one")["line_ok"]) == 1
    quirk = ls.scene("integer")
    _, pix = lm.sample_pixels(quirk["line_ends"][2], quirk["depth"].shape, ls.PARAMS)
    assert pix[0] == (0, 0) and pix[-1] == (39, 29)                      # integral (0, 0) clamps at 0; integral (30, 40) reads pixel (39, 29)


def test_margins():
    """Every scene, no exemptions: each dist < dist_thresh comparison at least 1e-9 (relative) from the threshold, each lambda * 10 at least
    1e-9 from the cell boundaries 1 .. 9 (0 and 10 are not boundaries: |.| folds what lies below 0 into cell 0, and [9, 10) shares the last
    cell with lambda >= 1 -- the two extreme samples always sit there), support ratio and length at least 1e-6 from theirs."""
    for name in ls.ALL_SCENES:
        for j, r in _lines(name):
            g = r["margins"]
            assert g["dist"] >= 1e-9 and g["cell"] >= 1e-9 and g["support"] >= 1e-6 and g["length"] >= 1e-6, (name, j, g)


# ---- selection ----------------------------------------------------------------------------------------------------------------------------
def _stereo_initialization(z, held, obs, ok):
    new = np.zeros(len(z), np.uint8)
    for i in range(len(z)):
        if z[i][0] > 0 and z[i][1] > 0:
            if not ok[i]:
                continue
            new[i] = 1
    return new


def _update_last_frame(z, held, obs, ok, limit=30):
    new = np.zeros(len(z), np.uint8)
    n_lines = 0
    for i in range(len(z)):
        if z[i][0] > 0 and z[i][1] > 0:
            create = False
            if not held[i]:
                create = True
            elif obs[i] < 1:
                create = True
            if create:
                if not ok[i]:
                    continue
                new[i] = 1
                n_lines += 1
            else:
                n_lines += 1
            if n_lines > limit:
                break
    return new


def _create_new_keyframe(z, held, obs, ok, limit=30):
    new = np.zeros(len(z), np.uint8)
    v = []
    for i in range(len(z)):
        if z[i][0] > 0 and z[i][1] > 0:
            v.append((float(min(z[i][0], z[i][1])), i))
    if v:
        v.sort()
        n_lines = 0
        for _, i in v:
            create = False
            if not held[i]:
                create = True
            elif obs[i] < 1:
                create = True
            if create:
                if not ok[i]:
                    continue
                new[i] = 1
                n_lines += 1
            else:
                n_lines += 1
            if n_lines > limit:
                break
    return new


@pytest.mark.parametrize("seed", range(12))
def test_selection_against_the_three_loops(seed):
    """Random line_ok / flag / depth patterns, with ties in the min depth and enough lines for the 31st-line stop (and too few for it)."""
    rng = np.random.default_rng(seed)
    n = int(rng.choice([0, 1, 20, 45, 120, 256]))
    z = rng.choice(np.array([-1.0, 0.0, 0.8, 1.0, 1.0, 1.5, 2.0, 2.0, 3.0], np.float32), (n, 2))
    held = rng.random(n) < 0.4
    obs = np.where(rng.random(n) < 0.6, 1, 0) * held
    flags = (held.astype(np.uint8) | (obs.astype(np.uint8) << 1)).astype(np.uint8)
    p_ok = (0.2, 0.9)[seed % 2]
    for order, loop in ((lm.ALL, _stereo_initialization), (lm.INDEX_ORDER, _update_last_frame), (lm.DEPTH_ORDER, _create_new_keyframe)):
        # line_ok as msl_lines_3d defines it: only candidates of the mode can carry a line
        cand = (z[:, 0] > 0) & (z[:, 1] > 0) & ((order == lm.ALL) | ~(held & (obs > 0)))
        ok = ((rng.random(n) < p_ok) & cand).astype(np.uint8)
        want = loop(z, held, obs, ok)
        got = lm.select(order, z, flags, ok, 30)
        assert np.array_equal(got, want), (seed, order)
        if order != lm.ALL and n == 256 and p_ok > 0.5:
            assert want.sum() < ok.sum()                                  # the stop was reached

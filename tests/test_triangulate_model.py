"""The scenes of tests/triangulate_scenes.py are discriminating, proved against the sequential model (tests/triangulate_model.py) alone: the
chain across neighbours matters, ties and shared idx2 occur, every reachable status code occurs, no decision sits on its threshold, and the
pinned eigen-solver stands in for cv::SVD.  No GPU."""
import numpy as np

from tests import triangulate_model as tm
from tests import triangulate_scenes as ts

# The largest relative difference |X_pin - X_svd| / |X_svd| of the dehomogenised point between the pinned solver (Jacobi on A^T A in
# double, vt.row(3) cast to float, float division) and numpy.linalg.svd (float64) of the same float A, measured over every triangulated
# candidate of every scene, limit_scene included.  It is the float rounding of the four components and of the
# division; the test allows 4x.
SVD_MEASURED = 1.13e-7
assert 4 * SVD_MEASURED <= 1e-5


def _items(name):
    s = ts.scene(name)
    return [(s, c, nb, res) for (c, nb), res in zip(s["items"], ts.model(name))]


def _all_items():
    return [(n,) + it for n in ts.ALL for it in _items(n)]


def test_model_outputs_are_consistent():
    """new_order lists every created idx1 once, in neighbour order then ascending idx1; a created point's status is a created code."""
    for name, s, c, nb, res in _all_items():
        order = res["new_order"]
        assert len(set(order.tolist())) == len(order), name
        key = [(int(res["new_neigh"][i]), int(i)) for i in order]
        assert key == sorted(key), name
        made = np.nonzero(res["new_neigh"] >= 0)[0]
        assert sorted(made.tolist()) == sorted(order.tolist())
        for i in made:
            r = res["new_neigh"][i]
            assert res["status"][r, i] in tm.CREATED and res["match12"][r, i] == res["new_idx2"][i]
            assert (res["new_desc"][i] == s["table"][nb[r]]["desc"][res["new_idx2"][i]]).all()
            # an idx1 that got its point is not searched again
            assert (res["match12"][r + 1:, i] == -1).all() and (res["status"][r + 1:, i][[not t["skipped"] for t in res["trace"][r + 1:]]] == tm.NO_MATCH).all()


def test_created_idx1_would_match_the_next_neighbour_too():
    hits = 0
    for name, s, c, nb, res in _all_items():
        if len(nb) < 2:
            continue
        free = tm.create_new_map_points(s["prm"], s["table"], c, nb, use_mask=False)
        i0 = np.nonzero(res["new_neigh"] == 0)[0]
        hits += int((free["match12"][1, i0] >= 0).sum())
    assert hits > 10


def test_ignoring_the_chain_changes_the_kept_bins():
    s = ts.scene("chain")
    (c, nb), res = s["items"][0], ts.model("chain")[0]
    free = tm.create_new_map_points(s["prm"], s["table"], c, nb, use_mask=False)
    assert set(res["trace"][1]["keep"]) == {3, 6, 9} and set(free["trace"][1]["keep"]) == {0, 3, 6}
    assert (res["match12"][1] != free["match12"][1]).any()
    # the same pair as a one-neighbour item is the unchained search
    alone = ts.model("chain")[1]
    assert (alone["match12"][0] == free["match12"][1]).all() and (alone["match12"][0] != res["match12"][1]).any()
    # and with the chain, a point of the dropped bin 9 is kept while the free run culls it
    i9 = np.nonzero(res["trace"][1]["bins"] == 9)[0]
    assert len(i9) and (res["match12"][1, i9] >= 0).all() and (free["match12"][1, i9] == -1).all()


def test_ties_go_to_the_later_idx2():
    s = ts.scene("special")
    res = ts.model("special")[0]
    tr = res["trace"][2]                                                  # neighbour 3 of the table
    assert len(tr["ties"]) >= 3
    tags2 = s["table"][3]["tags"]
    for idx1, earlier, later in tr["ties"]:
        assert later > earlier and {tags2[earlier], tags2[later]} == {"tie2a", "tie2b"}
        assert tr["before"][idx1] == later


def test_two_idx1_share_one_idx2_and_both_are_created():
    s = ts.scene("special")
    res = ts.model("special")[0]
    tags1 = s["table"][0]["tags"]
    ia = [i for i, t in enumerate(tags1) if t == "share1a"]; ib = [i for i, t in enumerate(tags1) if t == "share1b"]
    pairs = 0
    for a in ia:
        for b in ib:
            if res["new_idx2"][a] >= 0 and res["new_idx2"][a] == res["new_idx2"][b] and res["new_neigh"][a] == res["new_neigh"][b]:
                pairs += 1
    assert pairs == 3


def test_baseline_skip_epipole_rejection_and_node_lists():
    s = ts.scene("special")
    res = ts.model("special")[0]
    assert res["trace"][0]["skipped"] and (res["status"][0] == tm.NEIGHBOUR_SKIPPED).all() and res["nmatches"][0] == 0
    assert not any(t["skipped"] for t in res["trace"][1:])
    tags1, tags2 = s["table"][0]["tags"], s["table"][2]["tags"]
    rej = res["trace"][1]["epipole_rejects"]
    assert len(rej) >= 3 and all(tags1[a] == "epipole" and tags2[b] == "epipole" for a, b in rej)
    assert all(s["table"][0]["uright"][a] < 0 and s["table"][2]["uright"][b] < 0 for a, b in rej)
    assert all(res["trace"][1]["before"][a] == -1 for a, _ in rej)
    # nodes present on one side only, and features in no list, in the pair (0, 3)
    n1, n2 = s["table"][0]["node"], s["table"][3]["node"]
    assert set(n1[n1 >= 0]) - set(n2[n2 >= 0]) and set(n2[n2 >= 0]) - set(n1[n1 >= 0]) and (n1 == -1).any() and (n2 == -1).any()
    for i, t in enumerate(tags1):
        if t in ("only1", "nolist"):
            assert (res["match12"][:, i] == -1).all()


def test_every_reachable_status_occurs():
    """x3D(3) == 0 needs a null vector of A^T A with an exactly zero fourth component (a point at infinity hit exactly), and dist == 0 a
    triangulated point that is a camera centre to the last bit while its depth there is positive: neither is reachable from finite keypoints
    in general position, so the scenes do not force them (the kernel's branches for them are the model's)."""
    seen = set()
    for name, s, c, nb, res in _all_items():
        seen |= set(np.unique(res["status"]).tolist())
    assert seen == set(range(13)) - {tm.W_ZERO, tm.ZERO_DIST}, seen
    res = ts.model("special")[0]
    tags1 = ts.scene("special")["table"][0]["tags"]
    want = {"z1": tm.Z1, "z2": tm.Z2, "reproj1": tm.REPROJ1, "reproj2": tm.REPROJ2, "scale": tm.SCALE, "far": tm.LOW_PARALLAX, "axis0": tm.STEREO1,
            "axis1": tm.STEREO2, "axis2": tm.LOW_PARALLAX}
    for tag, code in want.items():
        idx = [i for i, t in enumerate(tags1) if t == tag]
        got = [int(res["status"][r, i]) for i in idx for r in range(len(res["status"])) if res["match12"][r, i] >= 0]
        assert got and all(g == code for g in got), (tag, code, got)


def test_margins():
    """No decision of any scene lies within 1e-3 (relative to its threshold's scale) of its threshold: baseline, epipole exclusion, epipolar
    line, the parallax tests (through 1 - cos), depths, reprojection errors, scale ratios, the 0.1 * max1 rules of the histogram."""
    total = 0
    for name in ts.ALL:
        for what, lhs, rhs, scale in ts.model_margins(name):
            total += 1
            assert abs(lhs - rhs) > 1e-3 * abs(scale), (name, what, lhs, rhs, scale)
    assert total > 5000


def _svd_figure(res):
    worst = 0.0
    for tr in res["trace"]:
        if tr["skipped"]:
            continue
        c = tr["cand"]
        m = c["tri"]
        if not m.any():
            continue
        vt = np.linalg.svd(c["A"][m].astype(np.float64))[2][:, 3, :]
        X = vt[:, :3] / vt[:, 3:4]
        Xm = (c["x3d"][m][:, :3] / c["x3d"][m][:, 3:4]).astype(np.float64)                    # the model's float division
        worst = max(worst, float((np.linalg.norm(X - Xm, axis=1) / np.linalg.norm(X, axis=1)).max()))
    return worst


def test_svd_pin_against_lapack():
    worst = max(_svd_figure(res) for name in ts.ALL for res in ts.model(name))
    s = ts.limit_scene()
    worst = max(worst, _svd_figure(tm.create_new_map_points(s["prm"], s["table"], *s["items"][0])))
    print("largest relative difference to numpy.linalg.svd:", worst)
    assert worst <= 4 * SVD_MEASURED

"""The sequential models of tests/mappoint_model.py agree with each other: the array form of msl_refresh_map_points / msl_covisibility
equals the literal statements on the object graph, on three keyframe graphs after a literal SearchInNeighbors; its descriptor choice
equals tests/fuse_model.py's where no keyframe is bad; the graph's observation table round-trips through the CSR arrays.  No GPU."""
import numpy as np
import pytest

from tests import fuse_scenes as fs
from tests import mappoint_model as mm
from tests import mappoint_scenes as ms


def _same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


@pytest.mark.parametrize("name", fs.ALL)
def test_array_model_equals_literal_refresh(name):
    g, prm = ms.graph(name)
    table, obs, points = mm.graph_table(g), mm.graph_observations(g), mm.graph_points(g)
    ids = list(range(len(g.mps)))
    got = mm.refresh_map_points(prm, table, obs, points, ids)
    seen = np.zeros(8, int)
    for f, mp in enumerate(g.mps):
        st = int(got["status"][f])
        seen += [st >> b & 1 for b in range(8)]
        before = (mp.desc.copy(), mp.normal.copy(), mp.dist.copy())
        pos = mm.compute_distinctive_descriptors(mp)
        wrote = mm.update_normal_and_depth(mp, prm)
        assert (pos is not None) == bool(st & mm.DESC_WRITTEN) and wrote == bool(st & mm.NORMAL_WRITTEN), (f, st)
        if pos is None:
            assert _same(mp.desc, before[0]) and got["best_obs"][f] == -1 and not got["out_desc"][f].any()
        else:
            assert _same(mp.desc, got["out_desc"][f]) and got["best_obs"][f] == pos
        if wrote:
            assert _same(mp.normal, got["out_normal"][f]) and _same(mp.dist, got["out_dist"][f])
        else:
            assert _same(mp.normal, before[1]) and _same(mp.dist, before[2]) and not got["out_normal"][f].any() and not got["out_dist"][f].any()
        assert bool(st & mm.BAD) == mp.bad and bool(st & mm.NO_OBS) == (not mp.bad and not mp.obs)
    # the graphs reach: written, bad (replaced) points, and descriptors chosen behind a bad keyframe
    assert seen[0] > 20 and seen[1] > 20 and seen[2] > 0
    assert any(got["best_obs"][f] > 0 and table[obs[f][0][0]]["bad"] for f in ids if got["status"][f] & mm.DESC_WRITTEN)


@pytest.mark.parametrize("name", fs.ALL)
def test_array_model_equals_literal_connections(name):
    g, _ = ms.graph(name)
    table, obs, points = mm.graph_table(g), mm.graph_observations(g), mm.graph_points(g)
    for th in (15, 3):
        kfs = list(range(len(g.kfs)))
        got = mm.covisibility(table, obs, points["flags"], kfs, th)
        for f, k in enumerate(kfs):
            lit = mm.update_connections(g.kfs[k], th)
            if lit is None:
                assert got["n_conn"][f] == 0 and not got["weight"][f].any()
                continue
            counter, lKFs, lWs = lit
            assert {j: int(w) for j, w in enumerate(got["weight"][f]) if w} == counter
            n = int(got["n_conn"][f])
            assert got["conn"][f, :n].tolist() == lKFs and got["conn_w"][f, :n].tolist() == lWs and (got["conn"][f, n:] == -1).all()
    assert (mm.covisibility(table, obs, points["flags"], [0], 3)["n_conn"] > 1).all()       # th = 3: a real ordered list


@pytest.mark.parametrize("name", fs.ALL)
def test_descriptor_choice_equals_fuse_model(name):
    g, prm = ms.graph(name)
    for kf in g.kfs:
        kf.bad = False
    table, obs, points = mm.graph_table(g), mm.graph_observations(g), mm.graph_points(g)
    got = mm.refresh_map_points(prm, table, obs, points, list(range(len(g.mps))), mm.REFRESH_DESC)
    fast = mm.refresh_map_points(prm, table, obs, points, list(range(len(g.mps))), mm.REFRESH_DESC, select=mm.select_descriptor_fast)
    assert all(_same(got[k], fast[k]) for k in got)
    n = 0
    for f, mp in enumerate(g.mps):
        if mp.bad or not mp.obs:
            continue
        mp.desc = np.full(32, 0xEE, np.uint8)
        mp.compute_distinctive_descriptors()
        assert _same(mp.desc, got["out_desc"][f]), f
        n += 1
    assert n > 30


def test_median_index_and_ties():
    r = np.random.RandomState(1)
    a = r.randint(0, 256, 32).astype(np.uint8)
    assert mm.select_descriptor([a]) == (0, 0) and mm.select_descriptor([a, (~a).astype(np.uint8)]) == (0, 0)
    assert [int(0.5 * (n - 1)) for n in (1, 2, 3, 4, 5)] == [0, 0, 1, 1, 2]
    for n in (3, 4, 5, 9, 40):
        d = [ms.desc_flip(a, r, r.randint(0, 30)) for _ in range(n)]
        assert mm.select_descriptor(d) == mm.select_descriptor_fast(d)
    s = ms.special()
    t = s["tags"]
    assert s["want"]["best_obs"][t["tie_later_rows"]] == 1 and s["want"]["best_obs"][t["all_equal"]] == 0
    assert s["want"]["best_obs"][t["bad_mixed"]] not in (0, 2) and s["want"]["best_obs"][t["bad_first_of_two"]] == 1


def test_csr_round_trip():
    from manhattanslam_amd import mappoint
    g, _ = ms.graph("a")
    obs = mm.graph_observations(g)
    o = mappoint.pack_observations(obs)
    assert o["obs_off"][0] == 0 and o["obs_off"][-1] == sum(len(x) for x in obs) and (np.diff(o["obs_off"]) >= 0).all()
    for pid, mp in enumerate(g.mps):
        b, e = o["obs_off"][pid], o["obs_off"][pid + 1]
        back = dict(zip(o["obs_kf"][b:e].tolist(), o["obs_idx"][b:e].tolist()))
        assert back == mp.obs and o["obs_kf"][b:e].tolist() == sorted(mp.obs)
    empty = mappoint.pack_observations([[], []])
    assert empty["obs_off"].tolist() == [0, 0, 0] and len(empty["obs_kf"]) == 1

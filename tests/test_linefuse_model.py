"""The ABI of msl_fuse_map_lines / msl_refresh_map_lines is sufficient, proved on the CPU models alone (tests/linefuse_model.py): the
batched entry-state results replayed in order against live objects leave exactly what the literal, sequential line half of
SearchInNeighbors leaves; the scenes of tests/linefuse_scenes.py reach every exit and keep every comparison off its threshold; the
candidate list is msl_fuse_candidates' and UpdateAverageDir agrees with a plain float64 formula.  No GPU."""
import numpy as np

from tests import fuse_model as fm
from tests import linefuse_model as lf
from tests import linefuse_scenes as ls

F32 = np.float32


def test_replay_equals_literal():
    """Batched model + replay == the literal function on three random keyframe graphs: slots, observation maps, nObs, bad flags,
    descriptors, mpReplaced, the refreshed normals and distances, and the return value of every Fuse call."""
    total = dict(REPLACED_BY_HELD=0, REPLACES_HELD=0, SELF=0, researched=0, UNRESOLVED=0, repeated=0, added_in_kf=0, checked=0)
    assert len(ls.ALL) >= 3
    for name in ls.ALL:
        R = ls.runs(name)
        (lit_rets, lit_snap), (rets, stats, snap) = R["literal"], R["replay"]
        assert rets == lit_rets, (name, rets, lit_rets)
        assert snap["slots"] == lit_snap["slots"], name
        assert snap["lines"] == lit_snap["lines"], name
        assert sum(rets) > 30, (name, rets)
        print(name, rets, stats)
        for k in total:
            total[k] += stats[k]
    assert total["REPLACED_BY_HELD"] >= 3 and total["REPLACES_HELD"] >= 3 and total["SELF"] >= 10, total
    assert total["researched"] >= 1 and total["repeated"] >= 1 and total["added_in_kf"] >= 1 and total["checked"] >= 50, total


def test_margins():
    """No comparison of any scene lies within 1e-3 (relative to its threshold's scale) of its threshold, the margin of
    tests/test_fuse_model.py::test_margins: the sign of both depths, the image bounds of both end points, the distance range, the view
    test, the integer PredictScale's ceil rounds to, and GetLinesInArea's midpoint and slope tests of every keyline.  The scenes have no
    non-finite values (tests/test_linefuse_gpu.py::test_edge_arithmetic places those by hand)."""
    total, kinds = 0, set()
    for name in ls.ALL:
        for what, lhs, rhs, scale in ls.margins(name):
            total += 1
            kinds.add(what)
            assert abs(lhs - rhs) > 1e-3 * abs(scale), (name, what, lhs, rhs, scale)
    assert total > 5000 and kinds >= {"z1", "z2", "minX", "maxX", "minY", "maxY", "minDistance", "maxDistance", "viewCos", "ceil", "area", "slope"}


def _seen(name):
    seen, added_in_kf, third = set(), 0, 0
    for table, lines, items, lists, res in ls.runs(name)["calls"]:
        for (t, l), r in zip(items, res):
            st = np.asarray(r["status"])
            seen |= set(st.tolist())
            added_in_kf += r["added_in_kf"]
            hit = st >= lf.ADDED
            slots = np.asarray(r["best_idx"])[hit]
            third += int((np.bincount(slots, minlength=1) >= 3).any()) if len(slots) else 0
    return seen, added_in_kf, third


def test_every_status_occurs():
    seen, added_in_kf, third = set(), 0, 0
    for name in ls.ALL:
        s, a, t = _seen(name)
        seen |= s; added_in_kf += a; third += t
        assert s == set(range(15)), (name, [lf.CODES[c] for c in set(range(15)) - s])
        assert a >= 1 and t >= 1, name
    assert added_in_kf >= 3 and third >= 3                                 # the add of a line already in the keyframe; a third hit on one slot
    # the keyframe sizes the scenes promise
    table = ls.runs("a")["entry"][0]
    assert max(len(k["kl"]) for k in table) == 256 and sorted(len(k["kl"]) for k in table)[-2] <= 40
    obs = ls.runs("a")["entry"][2]
    assert max(len(o) for o in obs) >= 4


def test_candidates_are_fuse_candidates():
    """The literal loop of src/LocalMapping.cc:589-605 == fuse_model.fuse_candidates (msl_fuse_candidates' model) over the line table."""
    for name in ls.ALL:
        g, p, cur, targets = ls.graph(name)
        for t in targets:
            lf.fuse_literal(p, g.kfs[t], list(g.kfs[cur].slots))
        want = [ml.id for ml in lf.line_candidates_literal(g, targets)]
        got, n = fm.fuse_candidates(g.table(), g.lines(), [list(targets)])[0]
        assert got == want and n == len(want) > 20, name
        assert ls.runs(name)["cand"][3][0][0] == want


def _plain_float64(table, xyz6, obs, ref, sf):
    """UpdateAverageDir written independently in numpy float64 (vectorised, np.linalg.norm, a float64 camera centre)."""
    P = np.asarray(xyz6, np.float64)
    mid = (P[:3] + P[3:]) / 2
    C = np.array([-np.asarray(table[k]["Tcw"], np.float64)[:, :3].T @ np.asarray(table[k]["Tcw"], np.float64)[:, 3] for k, _ in obs])
    V = mid[None, :] - C
    normal = (V / np.linalg.norm(V, axis=1)[:, None]).mean(0)
    Tr = np.asarray(table[ref]["Tcw"], np.float64)
    d = np.linalg.norm(mid - (-Tr[:, :3].T @ Tr[:, 3]))
    level = int(table[ref]["kl"]["octave"][dict(obs).get(ref, 0)])
    dmax = d * float(sf[level])
    return normal, np.array([dmax / float(sf[-1]), dmax])


def test_update_average_dir_against_float64():
    """The model's normal within 1e-15 relative and its distances within 2 ulp of float of a plain float64 formula (vectorised numpy,
    np.linalg.norm, mean).  The camera centres are inputs of UpdateAverageDir (KeyFrame::GetCameraCenter, float), so the formula gets
    the same centres widened to double; what is compared is the order and the precision of the model's sums and its float steps.  The
    scenes keep the end points exact in float (multiples of 2^-12), so the float midpoint is exact and the distance carries the
    roundings of the subtraction, the norm and the two scale factors only."""
    n = 0
    for name in ls.ALL:
        table, lines, obs = ls.runs(name)["entry"]
        p = ls.prm()
        # the plain formula with the keyframes' float centres widened, as the reference's objects hold them
        centred = []
        for k in table:
            T = np.asarray(k["Tcw"], F32)
            Ow = lf.gemm3(T, True, -1.0, T[:, 3]).astype(np.float64)
            T64 = np.concatenate([np.eye(3), -Ow[:, None]], 1)            # a pose with exactly this centre
            centred.append(dict(k, Tcw=T64))
        for i, o in enumerate(obs):
            if not o or not (lines["flags"][i] & 1):
                continue
            st, normal, dist = lf.update_average_dir(p, table, lines["xyz"][i], o, int(lines["ref"][i]))
            assert st == lf.NORMAL_WRITTEN
            want_n, want_d = _plain_float64(centred, lines["xyz"][i], o, int(lines["ref"][i]), p["scale_factors"])
            assert np.abs(normal - want_n).max() <= 1e-15 * np.abs(want_n).max(), (name, i, normal, want_n)
            ulp = np.spacing(want_d.astype(F32))
            assert (np.abs(dist.astype(np.float64) - want_d) <= 2 * ulp).all(), (name, i, dist, want_d)
            n += 1
    assert n > 100
    # the exits
    table, lines, obs = ls.runs("a")["entry"]
    i = next(i for i, o in enumerate(obs) if len(o) >= 2 and lines["flags"][i] & 1)
    assert lf.update_average_dir(ls.prm(), table, lines["xyz"][i], obs[i], 0, bad=True)[0] == lf.R_BAD
    assert lf.update_average_dir(ls.prm(), table, lines["xyz"][i], [], 0)[0] == lf.NO_OBS
    assert lf.update_average_dir(ls.prm(), table, lines["xyz"][i], obs[i], len(table))[0] == lf.BAD_OCTAVE


def test_slot_walk_table():
    """The rows of msl.h's slot walk on one slot: the self-hit leaves the state alone, the add of a line already in the keyframe adds no
    observation."""
    from manhattanslam_amd import KEYLINE_DTYPE
    kl = np.zeros(2, KEYLINE_DTYPE)
    kl["x"], kl["y"], kl["angle"], kl["octave"] = [160.0, 40.0], [120.0, 40.0], [0.5, 0.5], [0, 0]
    p = ls.prm()

    def kf(held):
        return dict(kl=kl, ldesc=np.zeros((2, 32), np.uint8), Tcw=np.eye(4, dtype=F32)[:3], held_id=np.array(held, np.int32))
    z = 3.0
    x = lambda u: (u - ls.CX) / ls.FX * z
    y = lambda v: (v - ls.CY) / ls.FY * z
    row = [x(150.0), y(120.0), z, x(170.0), y(120.0), z]
    d = float(np.linalg.norm([x(160.0), y(120.0), z]))
    n = 5
    lines = dict(xyz=np.array([row] * n), normal=np.array([[x(160.0) / d, y(120.0) / d, z / d]] * n), dist=np.array([[d * 0.95 / 1.2 ** 7, d * 0.95]] * n, F32),
                 desc=np.zeros((n, 32), np.uint8), flags=np.array([1, 1, 1, 1, 0], np.uint8), nobs=np.array([1, 2, 9, 9, 5], np.int32))
    r = lf.fuse_item(p, kf([-1, -1]), lines, [0, 1, 2])                      # ADDED (1 + 1 = 2), 2 > 2 false: REPLACES_HELD, then stale
    assert r["status"].tolist() == [lf.ADDED, lf.REPLACES_HELD, lf.UNRESOLVED] and r["other"].tolist() == [-1, 0, 1] and r["n_fused"] == 3
    r = lf.fuse_item(p, kf([-1, 0]), lines, [0, 1])                          # 0 is in the keyframe already: nobs stays 1, 1 > 2 false
    assert r["status"].tolist() == [lf.ADDED, lf.REPLACES_HELD] and r["added_in_kf"] == 1
    r = lf.fuse_item(p, kf([-1, -1]), lines, [1, 0])                         # 2 + 1 = 3 > 1: REPLACED_BY_HELD
    assert r["status"].tolist() == [lf.ADDED, lf.REPLACED_BY_HELD]
    r = lf.fuse_item(p, kf([1, -1]), lines, [1, 0, 2])                       # the self-hit changes nothing: 0 resolves from the entry state
    assert r["status"].tolist() == [lf.SELF, lf.REPLACED_BY_HELD, lf.UNRESOLVED] and r["other"].tolist() == [1, 1, 1] and r["n_fused"] == 3
    r = lf.fuse_item(p, kf([1, -1]), lines, [2, 1])                          # replaced first: the former holder's own hit is the caller's
    assert r["status"].tolist() == [lf.REPLACES_HELD, lf.UNRESOLVED] and r["other"].tolist() == [1, 2]
    r = lf.fuse_item(p, kf([4, -1]), lines, [0, -1, 4, 1])
    assert r["status"].tolist() == [lf.HELD_BAD, lf.NULL, lf.BAD, lf.HELD_BAD] and r["best_dist"].tolist() == [0, lf.INT_MAX, lf.INT_MAX, 0]

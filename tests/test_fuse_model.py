"""The ABI of msl_fuse_map_points / msl_fuse_candidates is sufficient, proved on the CPU models alone (tests/fuse_model.py): the batched
entry-state results replayed in order against live objects leave exactly what the literal, sequential SearchInNeighbors leaves; the
scenes of tests/fuse_scenes.py reach every exit and keep every comparison off its threshold; the pins of include/msl.h hold.  No GPU."""
import numpy as np

from tests import fuse_model as fm
from tests import fuse_scenes as fs
from tests.triangulate_scenes import KP

F32 = np.float32


def test_replay_equals_literal():
    """Batched model + replay == the literal function on three random keyframe graphs: slots, observation maps, nObs, bad flags,
    descriptors, mpReplaced and every return value."""
    total = dict(REPLACED_BY_HELD=0, REPLACES_HELD=0, researched=0, research_changed=0, UNRESOLVED=0)
    assert len(fs.ALL) >= 3
    for name in fs.ALL:
        R = fs.runs(name)
        (lit_rets, lit_snap), (rets, stats, snap) = R["literal"], R["replay"]
        assert rets == lit_rets, name
        assert snap["slots"] == lit_snap["slots"], name
        assert snap["points"] == lit_snap["points"], name
        assert sum(rets) > 50
        print(name, stats)
        for k in total:
            total[k] += stats[k]
    assert total["REPLACED_BY_HELD"] >= 5 and total["REPLACES_HELD"] >= 5, total
    assert total["researched"] >= 1 and total["research_changed"] >= 1, total     # a survivor searched again, and with another outcome
    assert total["UNRESOLVED"] >= 1, total


def test_margins():
    """No comparison of any scene lies within 1e-3 (relative to its threshold's scale) of its threshold, the margin of
    tests/test_triangulate_model.py::test_margins and for its reason: the image bounds, the distance range, the view cosine, the two
    chi-square bounds, the integer PredictScale's ceil rounds to, the sign of the depth."""
    total = 0
    for name in fs.ALL:
        for what, lhs, rhs, scale in fs.margins(name):
            total += 1
            assert abs(lhs - rhs) > 1e-3 * abs(scale), (name, what, lhs, rhs, scale)
    assert total > 5000


def _events(name):
    seen, chi, ties, clipped, equal = set(), set(), [], 0, 0
    bad_holder = 0
    for table, points, items, lists, res in fs.runs(name)["calls"]:
        for (t, l), r in zip(items, res):
            seen |= set(np.asarray(r["status"]).tolist())
            equal += r["equal_nobs"]
            for j, tr in enumerate(r["trace"]):
                chi |= tr.get("chi", set())
                ties += [x for x in tr.get("ties", []) if x[2] != x[3] and r["best_idx"][j] == x[0]]
                clipped += int(tr.get("clipped_corner", False) and tr["n_indices"] > 0)
            held = table[t]["held_id"]
            bad_holder += int(((held >= 0) & (points["flags"][np.maximum(held, 0)] == 0)).sum())
    return seen, chi, ties, clipped, equal, bad_holder


def test_scene_coverage():
    for name in fs.ALL:
        seen, chi, ties, clipped, equal, bad_holder = _events(name)
        assert seen == set(range(15)), (name, [fm.CODES[c] for c in set(range(15)) - seen])
        assert chi == {("stereo", True), ("stereo", False), ("mono", True), ("mono", False)}, name
        assert ties and all(w > l for w, l, _, _ in ties), name           # a Hamming tie across two cells: the earlier cell wins, not the index
        assert clipped >= 1 and equal >= 1 and bad_holder >= 1, name
        # windows of more than 64 cells occur (the wave walks them in two rounds)
        assert any(tr.get("cells", 0) > 64 for _, _, _, _, res in fs.runs(name)["calls"] for r in res for tr in r["trace"]), name


def test_candidates_model():
    for name in fs.ALL:
        table, points, items, res = fs.runs(name)["cand"]
        lst, n = res[0]
        assert n == len(lst) == len(set(lst)) > 100
        assert all(points["flags"][i] & 1 for i in lst)
        pos = {}
        for r, t in enumerate(items[0]):
            for s, h in enumerate(table[t]["held_id"]):
                if h >= 0 and points["flags"][h] & 1:
                    pos.setdefault(int(h), (r, s))
        assert lst == sorted(pos, key=pos.get)
        assert fm.fuse_candidates(table, points, items, lcap=10)[0] == (lst[:10], n)


# ---- pins -----------------------------------------------------------------------------------------------------------------------------------
def _kf(kps, held=None, T=None):
    """kps: rows (x, y, octave, uright, desc byte)."""
    kp = np.zeros(len(kps), KP)
    kp["x"] = [k[0] for k in kps]; kp["y"] = [k[1] for k in kps]; kp["octave"] = [k[2] for k in kps]
    return dict(kps_un=kp, uright=np.array([k[3] for k in kps], F32), grid_cell=np.array([fs.grid_cell(k[0], k[1]) for k in kps], np.int32),
                desc=np.array([[k[4]] * 32 for k in kps], np.uint8).reshape(len(kps), 32),
                Tcw=np.eye(4, dtype=F32)[:3] if T is None else T, held_id=np.array(held if held is not None else [-1] * len(kps), np.int32))


def _pts(rows):
    """rows: (u, v, z, desc byte, flags, nobs): a point at depth z behind pixel (u, v) of the identity camera, level 0 at that depth."""
    xyz = [((u - fs.CX) / fs.FX * z, (v - fs.CY) / fs.FY * z, z) for u, v, z, _, _, _ in rows]
    d = [np.linalg.norm(x) for x in xyz]
    return dict(xyz=np.array(xyz, F32), normal=np.array([np.array(x) / n for x, n in zip(xyz, d)], F32),
                dist=np.array([(n * 0.95 / 1.2 ** 7, n * 0.95) for n in d], F32), desc=np.array([[r[3]] * 32 for r in rows], np.uint8),
                flags=np.array([r[4] for r in rows], np.uint8), nobs=np.array([r[5] for r in rows], np.int32))


def test_pin_in_keyframe_is_read_from_the_table():
    """IsInKeyFrame(pKF) = id in held_id[tgt][:n_kps], whatever slot holds it and even if the point projects onto another keypoint."""
    kf = _kf([(80.0, 60.0, 0, -1.0, 0), (20.0, 20.0, 0, -1.0, 0)], held=[-1, 0])
    pts = _pts([(80.0, 60.0, 3.0, 0, 1, 2), (80.0, 60.0, 3.0, 0, 1, 2)])
    r = fm.fuse_item(fs.prm(), kf, pts, [0, 1])
    assert r["status"].tolist() == [fm.IN_KEYFRAME, fm.ADDED] and r["best_idx"].tolist() == [-1, 0] and r["n_fused"] == 1


def test_pin_octave_outside_the_pyramid_is_never_a_candidate():
    """Level 0 admits octave -1 by the reference's test (it would index mvInvLevelSigma2[-1]); pinned: not a candidate."""
    pts = _pts([(80.0, 60.0, 3.0, 0, 1, 2)])
    r = fm.fuse_item(fs.prm(), _kf([(80.0, 60.0, -1, -1.0, 0)]), pts, [0])
    assert r["trace"][0]["level"] == 0 and r["trace"][0]["n_indices"] == 1 and r["status"][0] == fm.NO_CANDIDATE and r["best_dist"][0] == 256
    r = fm.fuse_item(fs.prm(), _kf([(80.0, 60.0, 0, -1.0, 0)]), pts, [0])
    assert r["status"][0] == fm.ADDED


def test_pin_held_id_outside_the_point_table_is_an_empty_slot():
    pts = _pts([(80.0, 60.0, 3.0, 0, 1, 2)])
    r = fm.fuse_item(fs.prm(), _kf([(80.0, 60.0, 0, -1.0, 0)], held=[7]), pts, [0])
    assert r["status"][0] == fm.ADDED and r["other"][0] == -1


def test_pin_half_open_image_bounds_and_nonfinite_projection():
    p = fs.prm()
    kf = _kf([(80.0, 60.0, 0, -1.0, 0)])
    pts = _pts([(0.0, 60.0, 3.0, 0, 1, 2), (160.0, 60.0, 3.0, 0, 1, 2), (80.0, 60.0, 3.0, 0, 1, 2)])
    pts["xyz"][0] = [(0.0 - fs.CX) / fs.FX * 2.0, 0.0, 2.0]                # u == minX exactly: inside
    pts["xyz"][1] = [(160.0 - fs.CX) / fs.FX * 2.0, 0.0, 2.0]              # u == maxX exactly: outside
    pts["xyz"][2] = [0.5, 0.5, 0.0]                                         # z == 0: not behind, u = inf
    r = fm.fuse_item(p, kf, pts, [0, 1, 2])
    assert r["trace"][0]["u"] == 0.0 and r["trace"][1]["u"] == 160.0 and np.isinf(r["trace"][2]["u"])
    assert r["status"][0] not in (fm.OUT_OF_IMAGE, fm.BEHIND) and r["status"][1] == fm.OUT_OF_IMAGE and r["status"][2] == fm.OUT_OF_IMAGE


def test_slot_walk_table():
    """The rows of msl.h's slot walk, one slot, candidates in order."""
    kp = [(80.0, 60.0, 0, 80.0 - 8.0 / 3.0, 0)]                                          # a stereo keypoint: an added point gains 2 observations
    rows = [(80.0, 60.0, 3.0, 0, 1, n) for n in (1, 3, 9, 9)] + [(80.0, 60.0, 3.0, 0, 1, 5), (80.0, 60.0, 3.0, 0, 0, 5)]
    pts = _pts(rows)
    p = fs.prm()
    # empty: ADDED (nobs 1 + 2), then 3 > 3 is false: REPLACES_HELD, then stale: UNRESOLVED with the new holder
    r = fm.fuse_item(p, _kf(kp), pts, [0, 1, 2])
    assert r["status"].tolist() == [fm.ADDED, fm.REPLACES_HELD, fm.UNRESOLVED] and r["other"].tolist() == [-1, 0, 1] and r["n_fused"] == 3
    # empty: ADDED (nobs 3 + 2 = 5 > 1): REPLACED_BY_HELD, the holder stays
    r = fm.fuse_item(p, _kf(kp), pts, [1, 0, 2])
    assert r["status"].tolist() == [fm.ADDED, fm.REPLACED_BY_HELD, fm.UNRESOLVED] and r["other"].tolist() == [-1, 1, 1]
    # held by a good point with 5 observations: 5 > 3, 5 > 9 is false
    r = fm.fuse_item(p, _kf(kp, held=[4]), pts, [1, 2])
    assert r["status"].tolist() == [fm.REPLACED_BY_HELD, fm.UNRESOLVED] and r["other"].tolist() == [4, 4]
    r = fm.fuse_item(p, _kf(kp, held=[4]), pts, [2, 3])
    assert r["status"].tolist() == [fm.REPLACES_HELD, fm.UNRESOLVED] and r["other"].tolist() == [4, 2]
    # held by a bad point: counted, nothing done, for every hit
    r = fm.fuse_item(p, _kf(kp, held=[5]), pts, [0, 1, -1, 2])
    assert r["status"].tolist() == [fm.HELD_BAD, fm.HELD_BAD, fm.NULL, fm.HELD_BAD] and r["other"].tolist() == [5, 5, -1, 5] and r["n_fused"] == 3

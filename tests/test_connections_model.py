"""The sequential model of msl_connections_apply (tests/connections_model.py) against its literal twin on objects after every op of random
logs and of the hand-built scenes; what each pin of msl.h leaves, spelled out; the quirks the logs must reach; msl_fuse_targets' model
against its twin.  No GPU."""
import numpy as np
import pytest

from tests import connections_model as cm
from tests import connections_scenes as sc

U, B = cm.UPDATE, cm.KF_BAD


def stepwise(s, events=None):
    """The log one op at a time, model and twin side by side: the final state, and the statuses."""
    n = len(s["state"]["parent"])
    assert s["state"]["conn"].shape[1] == n
    st, kfs, status = cm.copy(s["state"]), cm.twin_from_state(s["state"], s["origin"]), []
    assert cm.twin_differences(kfs, st) == []
    weight = [] if s["weight"] is None else s["weight"]
    for i, op in enumerate(s["ops"]):
        r = cm.apply(st, weight, [op], s["origin"], s["th"], events=events)
        st, status = r["state"], status + r["op_status"]
        cm.twin_step(kfs, op, weight, s["th"])
        assert cm.twin_differences(kfs, st) == [], (i, op)
    return st, status


def stale_neighbour(st):
    """A live keyframe whose map holds a bad one (the state the quirk leaves; the event itself is raised by the model's KF_BAD, where a
    live keyframe holds the dying one and the dying one never held it)."""
    live = (st["kf_flags"] & cm.LIVE).astype(bool)
    return bool(((st["cw"] > 0) & live[:, None] & ~live[None, :]).any())


def test_array_model_equals_the_literal_twin_after_every_op_and_the_logs_reach_every_quirk():
    events, sizes, bad, below = set(), set(), 0, 0
    for seed in sc.RANDOM_SEEDS:
        s = sc.random_log(seed)
        n = len(s["state"]["parent"])
        assert 3 <= n <= 14 and 5 <= len(s["ops"]) <= 60
        sizes.add(n)
        st, status = stepwise(s, events)
        whole = sc.model(s)                                               # the log in one call leaves what the steps leave
        assert cm.same_state(whole["state"], st) and whole["op_status"] == status, seed
        assert whole["touched"] == sorted(set(whole["touched"])) and whole["counts"][0] == len(whole["touched"])
        assert whole["counts"][1] == int((~st["kf_flags"] & cm.LIVE).sum()) and whole["counts"][3] == 0
        bad += whole["counts"][1]
        below += int(((st["conn_w"] > 0) & (st["conn_w"] < s["th"])).sum())
    assert events == {"equal weight", "below th in a rebuilt row", "stale bad neighbour", "chained re-parenting", "leftover child"}
    assert sizes == set(range(3, 15)) and bad > 500 and below > 500


@pytest.mark.parametrize("make", [p for p in sc.PINS if p is not sc.pin_ccap_below_the_lists], ids=lambda p: p.__name__)
def test_the_hand_built_scenes_equal_the_twin_too(make):
    stepwise(make())


def rows(st):
    return [st["conn"][k][:min(st["n_conn"][k], st["conn"].shape[1])].tolist() for k in range(len(st["parent"]))]


def test_equal_weight_keeps_a_cut_row_and_a_changed_weight_brings_the_rest():
    r = sc.model(sc.pin_equal_weight_keeps_a_cut_row())
    assert rows(r["state"])[0] == [1] and r["state"]["cw"][0].tolist() == [0, 20, 3, 0] and r["op_status"] == [cm.DONE, cm.DONE | cm.PARENT_SET]
    assert rows(r["state"])[1] == [0, 3] and r["state"]["parent"].tolist() == [-1, 0, -1, -1] and r["touched"] == [0, 1, 3]
    r = sc.model(sc.pin_changed_weight_brings_the_entries_below_th())
    assert rows(r["state"])[0] == [1, 2] and r["state"]["conn_w"][0].tolist() == [21, 3, 0, 0]


def test_no_weight_reaches_th_and_equal_weights():
    r = sc.model(sc.pin_no_weight_reaches_th())
    assert rows(r["state"]) == [[2], [], [4, 0], [], [2]] and r["state"]["cw"][0].tolist() == [0, 0, 7, 7, 3]
    assert r["state"]["parent"].tolist() == [-1, -1, -1, -1, 2]
    r = sc.model(sc.pin_equal_weights_in_a_row())
    assert rows(sc.model(dict(sc.pin_equal_weights_in_a_row(), ops=[(U, 0, 0)]))["state"])[0] == [2, 5, 3, 1, 4]
    assert rows(r["state"])[0] == [2, 1, 5, 3, 4] and rows(r["state"])[1] == [2, 0, 5, 4]      # 1 sends INT32_MAX: row 0 rebuilt
    assert r["state"]["conn_w"][1][:2].tolist() == [2 ** 31 - 1] * 2


def test_one_directional_entry_survives_the_neighbour_s_kf_bad():
    r = sc.model(sc.pin_one_directional_entry_survives())
    st = r["state"]
    assert not st["kf_flags"][2] & cm.LIVE and st["cw"][0].tolist() == [0, 25, 3] and rows(st)[0] == [1, 2] and stale_neighbour(st)


def test_tree_loop():
    r = sc.model(sc.pin_tree_loop())
    assert r["state"]["parent"].tolist() == [-1, 0, 0, 0, 3, 0, 0, 4] and r["counts"] == [8, 1, 6, 0]
    assert rows(sc.pin_tree_loop()["state"])[7][:2] == [4, 3]             # 7 lists 4 before 3
    r = sc.model(sc.pin_tree_loop_without_a_parent())
    assert r["state"]["parent"].tolist() == [-1] * 8 and r["counts"] == [8, 1, 6, 0]


def test_early_returns_and_the_first_connection():
    r = sc.model(sc.pin_early_returns())
    assert r["op_status"] == [cm.KEPT, cm.KEPT, cm.DONE, cm.ALREADY_BAD, cm.ALREADY_BAD, cm.EMPTY, cm.DONE]
    assert r["state"]["parent"].tolist() == [-1, 0, 1, 1, 3] and r["counts"][1:3] == [1, 1]
    r = sc.model(sc.pin_first_connection_once())
    assert r["op_status"] == [cm.DONE | cm.PARENT_SET, cm.DONE, cm.DONE, cm.DONE] and r["state"]["parent"].tolist() == [-1, -1, 1, -1]
    assert r["state"]["kf_flags"].tolist() == [1, 1, 5, 1] and rows(r["state"])[2] == [3, 1, 0]


def test_ccap_below_the_lists():
    s = sc.pin_ccap_below_the_lists()
    assert s["state"]["conn"].shape[1] == 3 and s["state"]["n_conn"][0] == 7 and s["state"]["n_conn"][7] == 7
    assert s["state"]["conn"][7].tolist() == [6, 5, 4] and s["state"]["cw"][7][0] == 16       # 7 holds 0, beyond what its row stores
    r = sc.model(s)
    st = r["state"]
    assert st["n_conn"][0] == 1 and st["conn"][0].tolist() == [3, -1, -1] and st["conn"][3].tolist() == [0, 7, -1]
    assert st["n_conn"][7] == 6 and st["conn"][7].tolist() == [5, 4, 3] and st["parent"][7] == 0
    assert r["counts"] == [len(r["touched"]), 1, 1, 1] and r["touched"] == [0, 3, 5, 6, 7]


# ---- msl_fuse_targets --------------------------------------------------------------------------------------------------------------------
def test_fuse_targets_pins():
    """0's neighbours are 1, 2, 3.  1's neighbours are 4 (pushed), 2 (pushed as a second neighbour, not stamped), 0 (the current keyframe),
    5 (bad); 2 then comes again as a first neighbour, and its neighbours 4 (a second time) and 1 (stamped: skipped); 3 is bad.  For the
    current keyframe 1 the first neighbours 4, 2 and 0 are pushed and none of their neighbours: stamped, bad, or 1 itself."""
    s = cm.empty(6)
    for k, row in {0: [1, 2, 3], 1: [4, 2, 0, 5], 2: [4, 1]}.items():
        s["conn"][k][:len(row)], s["n_conn"][k] = row, len(row)
    s["kf_flags"][[3, 5]] = 0
    args = (s["conn"], s["n_conn"], s["kf_flags"], [0, 1])
    assert cm.fuse_targets(*args) == cm.fuse_targets_literal(*args) == [[1, 4, 2, 2, 4], [4, 2, 0]]
    assert cm.fuse_targets(*args, nn=1, nn2=2) == cm.fuse_targets_literal(*args, nn=1, nn2=2) == [[1, 4, 2], [4]]


def test_fuse_targets_model_equals_its_twin_on_the_graphs_the_logs_leave():
    longest = 0
    for seed in range(60):
        st = sc.model(sc.random_log(seed))["state"]
        n = len(st["parent"])
        for nn, nn2 in ((10, 5), (3, 2), (1, 1)):
            got = cm.fuse_targets(st["conn"], st["n_conn"], st["kf_flags"], range(n), nn, nn2)
            assert got == cm.fuse_targets_literal(st["conn"], st["n_conn"], st["kf_flags"], range(n), nn, nn2)
            longest = max(longest, max(map(len, got)))
    assert longest > 20

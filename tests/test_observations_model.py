"""The sequential model of msl_observations_apply (tests/observations_model.py) against its literal twin on objects, against the replay of
culled keyframes in tests/cull_model.py, and against the statements of the fusion replay in tests/fuse_model.py; five wrong
implementations told apart from the right one; the too-long rule.  No GPU."""
import numpy as np
import pytest

from tests import cull_model as cm
from tests import cull_scenes as cs
from tests import observations_model as om
from tests import observations_scenes as osc

SEEDS = osc.ALL_SEEDS


def scenes():
    return [(name, make()) for name, make in osc.all_scenes()]


def test_the_scenes_are_small_and_hold_every_case():
    kinds, cases = set(), set()
    for name, (s, ops) in scenes():
        n_tab, cap = s["held_id"].shape
        if name.startswith("random"):
            assert 4 <= n_tab <= 6 and 5 <= cap <= 8 and len(s["pt_flags"]) <= 40 and len(ops) <= 64, name
        kinds |= {o[0] for o in ops}
        assert sorted(ops, key=lambda o: o[0] != om.KF_ERASE) == list(ops), name       # every KF_ERASE in front (the sort is stable)
        for j, o in enumerate(ops):
            o = om.pad(o)
            if o[0] == om.REPLACE and any(q[0] == om.REPLACE and q[1] == o[2] for q in ops[j + 1:]):
                cases.add("chain")
            if o[0] == om.ADD and o in [om.pad(q) for q in ops[:j]]:
                cases.add("repeated add")
            if o[0] == om.ADD and not s["pt_flags"][o[1]] & 1:
                cases.add("add on a bad point")
            if o[0] == om.ERASE and s["pt_ref"][o[1]] == o[2] and any(k == o[2] for k, _ in s["obs"][o[1]]):
                cases.add("erase of the reference")
            if o[0] == om.ERASE and [k for k, _ in s["obs"][o[1]]] == [o[2]]:
                cases.add("erase of the last observation")
        for k in range(n_tab):
            held = [int(p) for p in s["held_id"][k][:s["n_kps"][k]] if p >= 0]
            if len(set(held)) < len(held):
                cases.add("held twice")
            if any(all(kk != k for kk, _ in s["obs"][p]) for p in held):
                cases.add("stale slot")
    assert kinds == {om.ADD, om.ERASE, om.SET_BAD, om.REPLACE, om.KF_ERASE}
    assert cases == {"chain", "repeated add", "add on a bad point", "erase of the reference", "erase of the last observation", "held twice",
                     "stale slot"}


@pytest.mark.parametrize("name,scene", scenes(), ids=[n for n, _ in scenes()])
def test_array_model_equals_the_literal_twin(name, scene):
    s, ops = scene
    want = om.apply(s, ops)
    assert want["counts"][2] == 0
    assert om.same_state(want["state"], om.apply_literal(s, ops)), name
    live = om.apply(s, ops, slots="live")                                 # KeyFrame::SetBadFlag's own walk: the same on every such scene
    assert om.same_state(want["state"], live["state"]) and (want["op_status"], want["touched"], want["counts"]) == (live["op_status"], live["touched"], live["counts"])
    assert len(want["op_status"]) == len(ops) and want["touched"] == sorted(set(want["touched"]))
    assert want["counts"][0] == sum(len(o) for o in want["state"]["obs"]) and want["counts"][1] == len(want["touched"])
    assert all(o == sorted(o) and len({k for k, _ in o}) == len(o) for o in want["state"]["obs"])


def test_the_pins_leave_what_msl_h_says():
    s, ops = osc.pin_erase_reference_and_last()
    w = om.apply(s, ops)
    assert w["state"]["pt_ref"].tolist() == [1, -1, -1] and w["op_status"] == [1, 0, 1, 0] and w["touched"] == [0, 1]
    s, ops = osc.pin_erase_cascade()
    w = om.apply(s, ops)
    assert w["op_status"] == [3, 1, 0, 1] and w["state"]["pt_nobs"].tolist() == [4, 3] and w["state"]["pt_flags"].tolist() == [4, 5]
    assert w["state"]["held_id"][0][0] == -1 and w["state"]["held_id"][1][2] == 0 and w["counts"] == [3, 2, 0, 1]
    s, ops = osc.pin_set_bad()
    w = om.apply(s, ops)
    assert w["op_status"] == [3, 0, 3] and w["state"]["pt_nobs"].tolist() == s["pt_nobs"].tolist() and (w["state"]["held_id"] == -1).all()
    s, ops = osc.pin_replace()
    w = om.apply(s, ops)
    assert w["op_status"] == [0, 3, 0] and w["state"]["obs"][1] == [(0, 0), (1, 2), (2, 0), (3, 3)] and w["state"]["pt_replaced"].tolist() == [1, -1, -1]
    assert w["state"]["held_id"][1][1] == -1 and w["state"]["held_id"][0][0] == 1 and (w["state"]["pt_found"][1], w["state"]["pt_visible"][1]) == (13, 27)
    s, ops = osc.pin_slot_written_twice()
    w = om.apply(s, ops)
    assert w["state"]["held_id"][1][1] == -1 and w["state"]["held_id"][2][0] == -1
    s, ops = osc.pin_add_new_and_known()
    w = om.apply(s, ops)
    assert w["state"]["obs"][0] == [(0, 2), (1, 0), (2, 3), (3, 1)] and w["state"]["held_id"][3][2] == 0 and w["op_status"] == [1, 1, 0, 1]


def test_the_pinned_difference_between_the_slots_on_entry_and_the_live_walk():
    """msl.h's pin on a hand-built scene: the literal twin is the live walk; the contract walks the slots on entry and turns one more
    point bad."""
    s, ops = osc.pin_kf_erase_inconsistent_pair()
    entry, live = om.apply(s, ops), om.apply(s, ops, slots="live")
    assert om.same_state(live["state"], om.apply_literal(s, ops)) and not om.same_state(entry["state"], live["state"])
    assert live["state"]["obs"][1] == [(1, 2), (2, 0)] and live["state"]["pt_flags"].tolist() == [4, 5] and live["op_status"] == [3, 0]
    assert entry["state"]["obs"][1] == [] and entry["state"]["pt_flags"].tolist() == [4, 4] and entry["op_status"] == [3, 3]
    assert entry["state"]["held_id"][2][0] == -1 and live["state"]["held_id"][2][0] == 1 and entry["counts"] == [0, 2, 0, 2]


@pytest.mark.parametrize("wrong", om.WRONG)
def test_a_wrong_implementation_is_told_apart(wrong):
    def differs(s, ops):
        return not om.same_state(om.apply(s, ops)["state"], om.apply(s, ops, wrong=wrong)["state"])
    assert any(differs(*pin()) for pin in osc.PINS), wrong
    assert any(differs(*osc.random_scene(seed)) for seed in SEEDS), wrong


# ---- against the culling model -------------------------------------------------------------------------------------------------------------
CULL_SCENES = [pin()[0] for pin in cs.PINS] + [cs.random_scene(seed, n_tab, cap, n_items=2) for seed, n_tab, cap in ((1, 8, 12), (2, 20, 30), (3, 12, 40))]


def test_a_kf_erase_log_is_the_replay_of_the_culled_keyframes():
    """[KF_ERASE(c) for c in order] leaves per point what cull_model.replay leaves on its objects: bad, nObs, observations -- that is, the
    walk over the slots with its cascades is KeyFrame::SetBadFlag's, and so is its expansion from the slots on entry."""
    n_culled = 0
    for scene in CULL_SCENES:
        for cand in scene["items"]:
            order = cm.cull_keyframes(scene, cand)[1]
            if not order:
                continue
            n_culled += len(order)
            s = osc.from_cull_scene(scene)
            w = om.apply(s, [(om.KF_ERASE, 0, c) for c in order])
            assert w["counts"][2] == 0
            got = [(not w["state"]["pt_flags"][p] & 1, int(w["state"]["pt_nobs"][p]), w["state"]["obs"][p]) for p in range(len(scene["pt_bad"]))]
            assert got == cm.replay(scene, order)
            # the expansion from the slots on entry: every ERASE the live walk makes, and no other that finds an observation
            flat = [(om.ERASE, int(p), c) for c in order for p in s["held_id"][c][:s["n_kps"][c]] if p >= 0]
            assert om.same_state(om.apply(s, flat)["state"], w["state"])
    assert n_culled > 20


# ---- against the fusion replay -------------------------------------------------------------------------------------------------------------
def test_the_recorded_fusion_log_leaves_the_graph_of_the_replay():
    from tests import fuse_scenes as fs
    kinds = set()
    for name in fs.ALL:
        entry, ops, g = osc.record_fuse_log(name)
        kinds |= {o[0] for o in ops}
        w = om.apply(entry, ops)
        assert w["counts"][2] == 0
        snap, st = g.snapshot(), w["state"]
        assert [[int(x) for x in st["held_id"][k][:st["n_kps"][k]]] for k in range(len(g.kfs))] == snap["slots"]
        for p, (obs, nobs, bad, _, replaced) in enumerate(snap["points"]):
            assert st["obs"][p] == sorted(obs.items()) and st["pt_nobs"][p] == nobs and bool(st["pt_flags"][p] & 1) == (not bad)
            assert st["pt_replaced"][p] == (-1 if replaced is None else replaced)
        assert om.same_state(st, osc.from_fuse_graph(g) | dict(pt_ref=st["pt_ref"]))
    assert kinds == {om.ADD, om.REPLACE}


# ---- too long ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(osc.LONG))
def test_too_long(name):
    s, ops = osc.long_map(), osc.LONG[name]
    assert s["held_id"].shape == (260, 2) and [len(o) for o in s["obs"]] == [256, 300, 255, 3, 0]
    w = om.apply(s, ops)
    assert w["counts"][2] == osc.LONG_COUNTS[name]
    if w["counts"][2]:
        assert om.same_state(w["state"], s) and w["counts"] == [814, 0, w["counts"][2], 0] and w["touched"] is None
    else:
        assert w["state"]["obs"][1] == s["obs"][1] and 1 not in w["touched"]       # the point of 300 is copied
        assert max(len(o) for p, o in enumerate(w["state"]["obs"]) if p != 1) == 256
        twin = osc.long_map(with_300=False)
        assert om.same_state(om.apply(twin, ops)["state"], om.apply_literal(twin, ops))

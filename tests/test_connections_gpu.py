"""msl_connections_apply and msl_fuse_targets on the GPU against tests/connections_model.py: every in-place array and every output
compared as bytes, in the device-memory, host-memory and _batch forms, with canaries around every device array; every pin on a hand-built
scene and the random logs of the model test; a state carried through four calls in device memory; the device-memory contract for ops,
weights and indices outside their tables; two runs of one log giving the same bytes; one run at the limits; and two chains in device
memory on one stream with nothing read back -- msl_covisibility into msl_connections_apply into msl_fuse_targets into
msl_fuse_candidates, and msl_covisibility into msl_connections_apply (UPDATE, then KF_BAD) into msl_local_keyframes."""
import numpy as np
import pytest

from tests import connections_model as cm
from tests import connections_scenes as sc

pytestmark = pytest.mark.gpu

U, B = cm.UPDATE, cm.KF_BAD
SCENES = sc.all_scenes()
D = sc.DevArray


@pytest.fixture(scope="module")
def matcher():
    from manhattanslam_amd.match import Matcher
    h = Matcher()
    yield h
    h.close()


def check(scene, matcher, forms=("device", "host", "batch"), tcap=None):
    """Every array equals the model's, in each form; returns the model's result."""
    a, sh = sc.pack(scene, tcap)
    want = sc.model(scene)
    e = sc.expected(sh, want)
    for form in forms:
        keep = {}
        got = sc.run(a, sh, mem=form == "device", handle=None if form == "batch" else matcher, keep=keep)
        diff = sc.same(got, e)
        assert diff == [], (form, {k: (got[k].tolist(), e[k].tolist()) for k in diff} if sh["n_tab"] <= 16 else diff)
        if form == "device":
            assert [k for k, v in keep.items() if not v.intact()] == []
    return want


@pytest.mark.parametrize("name,make", SCENES, ids=[n for n, _ in SCENES])
def test_every_scene_in_every_form(matcher, name, make):
    check(make(), matcher)


@pytest.mark.parametrize("seeds", sc.random_groups(), ids=lambda g: "seeds%d-%d" % (g[0], g[-1]))
def test_the_random_logs_of_the_model_test_in_every_form(matcher, seeds):
    """Every seed of tests/test_connections_model.py (connections_scenes.RANDOM_SEEDS), fifty to a case."""
    for seed in seeds:
        check(sc.random_log(seed), matcher)


def test_tcap_below_the_touched_count_and_larger_logs(matcher):
    """tcap = 1 under eight touched keyframes: the count stays full; and logs of 60 ops on 24 and 40 keyframes, more than one wave wide."""
    want = check(sc.pin_tree_loop(), matcher, tcap=1)
    assert want["counts"][0] == 8
    for seed, n in ((3, 24), (4, 40), (5, 33)):
        want = check(sc.random_log(seed, n_tab=n, n_ops=60), matcher, tcap=5)
        assert want["counts"][0] > 5 and want["counts"][1] > 0


def test_a_state_carried_through_four_calls_in_device_memory(matcher):
    """One log of 60 ops on 14 keyframes in four calls on the same device arrays, nothing copied in between: every call's outputs are the
    model's for its part, and the state at the end is the model's for the whole log."""
    from manhattanslam_amd import connections as cn
    scene = sc.random_log(2, n_tab=14, n_ops=60)
    a, sh = sc.pack(scene)
    d = {k: D(a[k]) for k in cn.INOUT_KEYS + ("weight",)}
    st, parts, keep = scene["state"], [scene["ops"][i:i + 15] for i in range(0, 60, 15)], []
    for ops in parts:
        want = cm.apply(st, scene["weight"], ops, scene["origin"], scene["th"])
        st = want["state"]
        d["ops"] = D(cn.pack_ops(ops))
        out = cn.outputs(len(ops), sh["tcap"], sc.device_filled)
        cn.apply_device(matcher, sh["n_tab"], sh["ccap"], sh["n_rows"], len(ops), sh["tcap"], sh["origin"], sh["th"], d, d, out)
        keep.append((d["ops"], out, sc.expected(dict(sh, n_ops=len(ops)), want)))
    matcher.sync()
    for ops_dev, out, e in keep:
        got = {k: v.numpy() for k, v in out.items()}
        assert sc.same(got, {k: e[k] for k in cn.OUT_KEYS}) == [] and all(v.intact() for v in out.values()) and ops_dev.intact()
    assert sc.same({k: d[k].numpy() for k in cn.INOUT_KEYS}, sc.model(scene)["state"]) == [] and all(v.intact() for v in d.values())
    assert sc.model(scene)["counts"][1] > 2


def test_ops_weights_and_indices_outside_their_tables(matcher):
    """The device-memory contract: an op with an unknown code or a field outside its table gets status 0; a negative weight is absent; an
    n_conn outside the row is clamped, a conn entry outside the table is no link, a parent outside the table makes no candidate; and the
    canaries around every array stay (check asks that of every device-memory run)."""
    scene = sc.random_log(6, n_tab=12, n_ops=40)
    n = 12
    bad = [(0, 1, 1), (3, 1, 1), (U, n, 0), (U, -1, 0), (U, 0, n), (U, 0, -1), (B, n), (B, -5), (-1, 0, 0), (1 << 30, 0, 0)]
    mixed = [x for pair in zip(scene["ops"], bad * 4) for x in pair]
    scene["weight"][scene["weight"] == 3] = -3
    half = sc.model(dict(scene, ops=scene["ops"][:20]))["state"]                # a graph to break
    half["cw"][half["cw"] == 14] = -14
    half["n_conn"][3], half["n_conn"][4] = -2, 1 << 20
    half["conn"][5][0], half["conn"][6][:] = n + 3, -7
    half["parent"][7], half["parent"][8] = n, -9
    want = check(dict(scene, state=half, ops=mixed), matcher, forms=("device",))
    assert [st for st, o in zip(want["op_status"], mixed) if o in bad] == [0] * 40 and sum(1 for s_ in want["op_status"] if s_ & cm.DONE) > 10


def test_two_runs_give_the_same_bytes(matcher):
    scene = sc.random_log(9, n_tab=40, n_ops=60)
    a, sh = sc.pack(scene)
    one, two = (sc.run(a, sh, mem=1, handle=matcher) for _ in range(2))
    assert sc.same(one, two) == [] and sc.same(one, sc.expected(sh, sc.model(scene))) == []


def test_the_limits(matcher):
    """n_tab = 4096, MSL_CONN_MAX_OPS ops, an UPDATE whose row has 4095 non-zero weights into pre-filled rows, and a KF_BAD of a keyframe
    with 300 children that chain (tests/connections_scenes.py: limits_scene)."""
    scene = sc.limits_scene()
    a, sh = sc.pack(scene)
    assert sh["n_tab"] == cm.MAX_TAB and sh["n_ops"] == cm.MAX_OPS and int((scene["weight"][0][:-1] > 0).sum()) == cm.MAX_TAB - 1
    assert int((scene["weight"][0] < scene["th"]).sum()) > 1000 and int((scene["state"]["parent"] == 1).sum()) == 300
    want = sc.model(scene)
    assert want["state"]["parent"][2:302].tolist() == list(range(3, 302)) + [0] and want["counts"][1] > 300 and want["counts"][2] > 600
    keep = {}
    got = sc.run(a, sh, mem=1, handle=matcher, keep=keep)
    assert sc.same(got, sc.expected(sh, want)) == [] and [k for k, v in keep.items() if not v.intact()] == []


# ---- msl_fuse_targets --------------------------------------------------------------------------------------------------------------------
def test_fuse_targets_in_every_form(matcher):
    """The graphs the random logs leave, every keyframe as the current one; tcap below the longest list; nn and nn2 at and below the rows."""
    longest = 0
    for seed in (1, 2, 7, 15):
        st = sc.model(sc.random_log(seed, n_tab=14, n_ops=40))["state"]
        cur = list(range(14))
        for nn, nn2, tcap in ((10, 5, 60), (10, 5, 7), (3, 2, 9), (1, 1, 1), (14, 14, 200)):
            e = sc.targets_expected(cm.fuse_targets(st["conn"], st["n_conn"], st["kf_flags"], cur, nn, nn2), len(cur), tcap)
            for form in ("device", "host", "batch"):
                keep = {}
                got = sc.run_targets(st, cur, nn, nn2, tcap, mem=form == "device", handle=None if form == "batch" else matcher, keep=keep)
                assert sc.same(got, e) == [], (seed, nn, nn2, tcap, form)
                assert form != "device" or all(v.intact() for v in keep.values())
            longest = max(longest, int(e["n_targets"].max()))
    assert longest > 20                                                   # lists beyond tcap = 7 and 9, and beyond n_tab


def test_fuse_targets_with_indices_outside_the_table(matcher):
    """Device memory: a cur outside the table has no targets, a conn entry outside it is no neighbour, an n_conn outside the row is clamped."""
    st = sc.model(sc.random_log(2, n_tab=14, n_ops=40))["state"]
    st["conn"][9][1], st["conn"][11][0], st["n_conn"][6], st["n_conn"][12] = 14, -1, 1 << 20, -4
    cur = [9, 11, 6, 12, 14, -1, 4]
    e = sc.targets_expected(cm.fuse_targets(st["conn"], st["n_conn"], st["kf_flags"], cur, 10, 5), len(cur), 40)
    keep = {}
    assert sc.same(sc.run_targets(st, cur, 10, 5, 40, mem=1, handle=matcher, keep=keep), e) == [] and all(v.intact() for v in keep.values())
    assert e["n_targets"].tolist()[3:6] == [0, 0, 0] and e["n_targets"][:3].min() > 5


# ---- the chains ----------------------------------------------------------------------------------------------------------------------------
def covisibility_on_device(matcher, m, d):
    """msl_covisibility of the map's new keyframe on the device tables: its outputs (weight is the row MSL_CONN_UPDATE reads)."""
    from manhattanslam_amd import mappoint
    n_tab, cap = m["held_id"].shape
    o = mappoint.pack_observations(m["obs"])
    d.update(held_id=D(m["held_id"]), n_kps=D(m["n_kps"]), pt_flags=D(m["pt_flags"]), obs_off=D(o["obs_off"]), obs_kf=D(o["obs_kf"]),
             kf=D(np.array([m["cur"]], np.int32)))
    cout = {k: D(v) for k, v in mappoint.covisibility_outputs(1, n_tab, n_tab).items()}
    mappoint.covisibility_device(matcher, n_tab, cap, len(m["obs"]), 1, int(o["obs_off"][-1]), n_tab, m["th"], d["held_id"], d["n_kps"], d["pt_flags"],
                                 d["obs_off"], d["obs_kf"], d["kf"], cout)
    return cout, int(o["obs_off"][-1])


def test_chain_covisibility_to_fuse_candidates_in_device_memory(matcher):
    from manhattanslam_amd import connections as cn
    from manhattanslam_amd._lib import MSL_MEM_DEVICE, check as ok, lib, ptr
    from tests import fuse_model as fm
    from tests import mappoint_model as mm
    m = sc.chain_map(31)
    n_tab, cap = m["held_id"].shape
    n_pts, cur, th, tcap, lcap = len(m["obs"]), m["cur"], m["th"], 60, 400
    cov = mm.covisibility(m["table"], m["obs"], m["pt_flags"], [cur], th=th, ccap=n_tab)
    ops = [(U, cur, 0)]
    want = cm.apply(m["state"], cov["weight"], ops, 0, th)
    st = want["state"]
    targets = cm.fuse_targets(st["conn"], st["n_conn"], st["kf_flags"], [cur])
    cand, n_cand = fm.fuse_candidates(m["table"], dict(flags=m["pt_flags"]), targets, lcap)[0]
    assert want["op_status"] == [cm.DONE | cm.PARENT_SET] and 10 < len(targets[0]) <= tcap and len(set(targets[0])) < len(targets[0]) and n_cand > 50

    d = {k: D(v) for k, v in m["state"].items()}
    cout, _ = covisibility_on_device(matcher, m, d)
    d.update(weight=cout["weight"], ops=D(cn.pack_ops(ops)), cur=d["kf"])
    out = cn.outputs(1, n_tab, sc.device_filled)
    cn.apply_device(matcher, n_tab, n_tab, 1, 1, n_tab, 0, th, d, d, out)
    tout = cn.targets_outputs(1, tcap, sc.device_filled)
    cn.fuse_targets(n_tab, n_tab, 1, 10, 5, tcap, d, tout, MSL_MEM_DEVICE, handle=matcher)
    fout = dict(cand=D(shape=(1, lcap), dtype=np.int32), n_cand=D(shape=(1,), dtype=np.int32))
    ok(lib.msl_fuse_candidates(matcher.h, n_tab, cap, n_pts, 1, tcap, lcap, ptr(d["held_id"]), ptr(d["n_kps"]), ptr(d["pt_flags"]), ptr(tout["targets"]),
                               ptr(tout["n_targets"]), MSL_MEM_DEVICE, ptr(fout["cand"]), ptr(fout["n_cand"]), MSL_MEM_DEVICE), "msl_fuse_candidates")
    matcher.sync()
    assert sc.same({k: v.numpy() for k, v in cout.items()}, cov) == []
    got = {k: d[k].numpy() for k in cn.INOUT_KEYS}
    got.update({k: v.numpy() for k, v in out.items()})
    assert sc.same(got, sc.expected(dict(n_ops=1, tcap=n_tab), want)) == []
    assert sc.same({k: v.numpy() for k, v in tout.items()}, sc.targets_expected(targets, 1, tcap)) == []
    assert fout["n_cand"].numpy().tolist() == [n_cand] and fout["cand"].numpy()[0][:len(cand)].tolist() == cand
    assert all(v.intact() for v in list(d.values()) + list(cout.values()) + list(out.values()) + list(tout.values()) + list(fout.values()))


def test_chain_covisibility_update_and_kf_bad_to_local_keyframes_in_device_memory(matcher):
    """The new keyframe is connected, then the parent it got is culled, and a frame that holds the new keyframe's points builds its local
    keyframes from conn, n_conn, parent and kf_flags as msl_connections_apply left them."""
    from manhattanslam_amd import connections as cn, localmap
    from tests import localmap_model as lm
    from tests import mappoint_model as mm
    m = sc.chain_map(32)
    n_tab, cap = m["held_id"].shape
    n_pts, cur, th = len(m["obs"]), m["cur"], m["th"]
    cov = mm.covisibility(m["table"], m["obs"], m["pt_flags"], [cur], th=th, ccap=n_tab)
    culled = int(cov["conn"][0][0])                                       # the parent the first connection gives
    ops = [(U, cur, 0), (B, culled)]
    want = cm.apply(m["state"], cov["weight"], ops, 0, th)
    st = want["state"]
    assert culled != 0 and want["op_status"] == [cm.DONE | cm.PARENT_SET, cm.DONE] and st["parent"][cur] not in (-1, culled)
    held = [int(p) for p in m["held_id"][cur][:m["n_kps"][cur]]]
    conn = [st["conn"][k][:st["n_conn"][k]].tolist() for k in range(n_tab)]
    loc = lm.update_local_keyframes(list(held), [not f & 1 for f in m["pt_flags"]], [[k for k, _ in o] for o in m["obs"]],
                                    [not f & cm.LIVE for f in st["kf_flags"]], conn, [None if p < 0 else int(p) for p in st["parent"]], [])
    assert culled not in loc["local_kf"] and len(loc["local_kf"]) > 4

    d = {k: D(v) for k, v in m["state"].items()}
    cout, n_obs = covisibility_on_device(matcher, m, d)
    d.update(weight=cout["weight"], ops=D(cn.pack_ops(ops)))
    out = cn.outputs(2, n_tab, sc.device_filled)
    cn.apply_device(matcher, n_tab, n_tab, 1, 2, n_tab, 0, th, d, d, out)
    d.update(cur_held=D(m["held_id"][cur:cur + 1]), n_cur=D(m["n_kps"][cur:cur + 1]))
    lout = localmap.keyframes_outputs(1, cap, n_tab, sc.device_filled)
    localmap.local_keyframes_device(matcher, 1, cap, n_tab, n_pts, n_obs, n_tab, d, lout)
    matcher.sync()
    got = {k: d[k].numpy() for k in cn.INOUT_KEYS}
    got.update({k: v.numpy() for k, v in out.items()})
    assert sc.same(got, sc.expected(dict(n_ops=2, tcap=n_tab), want)) == []
    e = dict(votes=np.zeros((1, n_tab), np.int32), local_kf=np.full((1, n_tab), -1, np.int32), n_local_kf=np.array([len(loc["local_kf"])], np.int32),
             ref_kf=np.array([-1 if loc["ref_kf"] is None else loc["ref_kf"]], np.int32), cur_cleared=np.zeros((1, cap), np.uint8),
             status=np.array([loc["status"]], np.uint8))
    for k, v in loc["votes"].items():
        e["votes"][0, k] = v
    e["local_kf"][0, :len(loc["local_kf"])] = loc["local_kf"]
    e["cur_cleared"][0, loc["cleared"]] = 1
    assert sc.same({k: v.numpy() for k, v in lout.items()}, e) == []
    assert all(v.intact() for v in list(d.values()) + list(cout.values()) + list(out.values()) + list(lout.values()))

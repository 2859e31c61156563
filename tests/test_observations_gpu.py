"""msl_observations_apply on the GPU against tests/observations_model.py: every in-place array, the new CSR table, op_status, touched and
counts, compared as bytes, in the host-memory and the device-memory form; every pin on a hand-built scene; the too-long scenes, where the
caller's arrays keep their bytes; the device-memory contract for ops outside their tables, with canaries around every array; one run at
the limits that matter to the kernels (65536 ADDs on distinct new rows up to keypoint 8191 with tcap 1, and a log of 256 KF_ERASE); two runs
of one log giving the same bytes; and two chains in device memory on one stream -- the recorded fusion log into msl_refresh_map_points and
msl_covisibility, and the culled keyframes of msl_cull_keyframes into a second msl_cull_keyframes."""
import numpy as np
import pytest

from tests import cull_model as cm
from tests import cull_scenes as cs
from tests import observations_model as om
from tests import observations_scenes as osc

pytestmark = pytest.mark.gpu

SCENES = osc.all_scenes() + [("pin_kf_erase_inconsistent_pair", osc.pin_kf_erase_inconsistent_pair)]   # the model suite's list, and the pin


@pytest.fixture(scope="module")
def matcher():
    from manhattanslam_amd.match import Matcher
    h = Matcher()
    yield h
    h.close()


def check(state, ops, matcher, forms=("device", "host", "batch"), **shape):
    """Every array equals the model's, in each form; returns the model's result."""
    a, sh = osc.pack(state, ops, **shape)
    want = om.apply(state, ops)
    e = osc.expected(a, sh, want)
    for form in forms:
        keep = {}
        got = osc.run(a, sh, mem=form == "device", handle=None if form == "batch" else matcher, keep=keep)
        diff = osc.same(got, e)
        assert diff == [], (form, {k: (got[k].tolist(), e[k].tolist()) for k in diff} if sh["n_pts"] <= 40 else diff)
        if form == "device":
            assert [k for k, v in keep.items() if not v.intact()] == []
    return want


@pytest.mark.parametrize("name,make", SCENES, ids=[n for n, _ in SCENES])
def test_every_scene_in_every_form(matcher, name, make):
    s, ops = make()
    check(s, ops, matcher)


@pytest.mark.parametrize("name", sorted(osc.LONG))
def test_too_long_scenes_keep_the_caller_s_bytes(matcher, name):
    """The device-memory form on the map with its untouchable point of 300 (a range with repeated keyframes, which a host-memory call
    refuses), the host-memory forms on the same map without it."""
    want = check(osc.long_map(), osc.LONG[name], matcher, forms=("device",))
    assert want["counts"][2] == osc.LONG_COUNTS[name]
    if not want["counts"][2]:
        assert want["state"]["obs"][1] == osc.long_map()["obs"][1]
    check(osc.long_map(with_300=False), osc.LONG[name], matcher, forms=("host", "batch"))


def test_ops_outside_their_tables_do_nothing_and_nothing_is_written_outside(matcher):
    """The device-memory contract: an op with an unknown code or a field outside its table gets status 0, a held_id outside the point table
    is skipped by KF_ERASE, and the canaries around every array stay (check asks that of every device-memory run)."""
    s, ops = osc.random_scene(7)
    n_tab, cap = s["held_id"].shape
    n_pts = len(s["pt_flags"])
    s["held_id"][s["held_id"] == -1] = np.resize([n_pts, -7, 1 << 30], (s["held_id"] == -1).sum())
    s["n_kps"][0] = cap + 3                                               # clamped
    bad = [(0, 1, 1, 0), (6, 1, 1, 0), (om.ADD, n_pts, 0, 0), (om.ADD, 0, n_tab, 0), (om.ADD, 0, 1, int(s["n_kps"][1])), (om.ADD, 0, 1, -1),
           (om.ERASE, -1, 0), (om.ERASE, 0, -1), (om.SET_BAD, 1 << 30), (om.REPLACE, 0, n_pts), (om.REPLACE, -2, 0), (om.KF_ERASE, 0, n_tab)]
    mixed = [x for pair in zip(ops, bad * 6) for x in pair]
    want = check(s, mixed, matcher, forms=("device",))
    assert [st for st, o in zip(want["op_status"], mixed) if o in bad] == [0] * len(ops) and any(want["op_status"])


def test_the_limits_that_matter_to_the_kernels(matcher):
    """65536 ADDs, each on a new row of its own, through every keypoint index up to 8191 of eight keyframes, with tcap = 1 and 65536 points
    touched; then one log of 256 KF_ERASE over a map of 256 keyframes."""
    n = om.MAX_OPS
    s = osc.empty(8, 8192, n + 3)
    osc.observe(s, n, 0, 5); osc.observe(s, n + 2, 7, 8191)                # old rows among the new ones; row n + 1 stays empty
    ops = [(om.ADD, p, p % 8, p // 8) for p in range(n)]
    want = check(s, ops, matcher, forms=("device", "host"), tcap=1)
    assert want["counts"] == [n + 2, n, 0, 0] and want["touched"][:2] == [0, 1]
    s, ops = osc.random_scene(11, n_tab=256, cap=6, n_pts=400, n_ops=300)
    ops = [(om.KF_ERASE, 0, int(k)) for k in np.random.default_rng(3).permutation(256)] + [o for o in ops if o[0] != om.KF_ERASE][:44]
    want = check(s, ops, matcher, forms=("device", "host"))
    assert [o[0] for o in ops].count(om.KF_ERASE) == om.MAX_KF_ERASE and want["counts"][3] > 20


def test_two_runs_give_the_same_bytes(matcher):
    s, ops = max((osc.random_scene(seed) for seed in range(10)), key=lambda x: len(x[0]["pt_flags"]) * len(x[1]))
    a, sh = osc.pack(s, ops)
    one, two = (osc.run(a, sh, mem=1, handle=matcher) for _ in range(2))
    assert osc.same(one, two) == [] and osc.same(one, osc.expected(a, sh, om.apply(s, ops))) == []


# ---- the chains ----------------------------------------------------------------------------------------------------------------------------
def test_chain_fusion_log_to_refresh_and_covisibility_in_device_memory(matcher):
    """The recorded log of the fusion replay applied to the device tables; then, with nothing read back, msl_refresh_map_points with ids =
    touched and n_items = tcap (the ids behind the count are -1: bad points) and msl_covisibility of the current keyframe on the new table,
    with n_obs_total = ocap.  Against the models run on the model's tables."""
    from manhattanslam_amd import mappoint, observations as ob
    from tests import fuse_scenes as fs
    from tests import mappoint_model as mm
    entry, ops, g = osc.record_fuse_log("a")
    a, sh = osc.pack(entry, ops)
    n_tab, cap, n_pts, tcap, ocap = sh["n_tab"], sh["cap"], sh["n_pts"], sh["tcap"], sh["ocap"]
    want = om.apply(entry, ops)
    st = want["state"]
    assert {o[0] for o in ops} == {om.ADD, om.REPLACE} and 0 < len(want["touched"]) < tcap
    table = [dict(desc=kf.data["desc"]) for kf in g.kfs]
    ids = np.array((want["touched"] + [-1] * tcap)[:tcap], np.int32)
    ref = mm.refresh_map_points(None, table, st["obs"], dict(flags=st["pt_flags"]), np.maximum(ids, 0), what=mm.REFRESH_DESC, select=mm.select_descriptor_fast)
    for f in np.nonzero(ids < 0)[0]:
        ref["out_desc"][f], ref["best_obs"][f], ref["best_median"][f], ref["status"][f] = 0, -1, 0, mm.BAD
    cov = mm.covisibility([dict(held_id=r[:n]) for r, n in zip(st["held_id"], st["n_kps"])], st["obs"], st["pt_flags"], [fs.CUR], th=5, ccap=n_tab)
    assert (ref["status"] & mm.DESC_WRITTEN).sum() > 3 and cov["n_conn"][0] > 0

    D = osc.DevArray
    d = {k: None if v is None else D(v) for k, v in a.items()}
    out = ob.outputs(n_pts, sh["n_ops"], ocap, tcap, osc.device_filled)
    ob.apply_device(matcher, n_tab, cap, n_pts, sh["n_obs_total"], sh["n_ops"], ocap, tcap, d, d, out)
    _, t = mappoint.pack_table(table, cap)
    dt = dict(desc=D(t["desc"]), n_kps=d["n_kps"], kf_flags=D(t["kf_flags"]))
    new = dict(obs_off=out["obs_off_out"], obs_kf=out["obs_kf_out"], obs_idx=out["obs_idx_out"])
    rout = {k: D(v) for k, v in mappoint.refresh_outputs(tcap).items()}
    mappoint.refresh_map_points_device(matcher, mappoint.refresh_params(mm.params()["scale_factors"]), n_tab, cap, n_pts, tcap, ocap, mm.REFRESH_DESC,
                                       dt, new, dict(pt_flags=d["pt_flags"]), out["touched"], rout, {})
    cout = {k: D(v) for k, v in mappoint.covisibility_outputs(1, n_tab, n_tab).items()}
    mappoint.covisibility_device(matcher, n_tab, cap, n_pts, 1, ocap, n_tab, 5, d["held_id"], d["n_kps"], d["pt_flags"], new["obs_off"], new["obs_kf"],
                                 D(np.array([fs.CUR], np.int32)), cout)
    matcher.sync()
    got = {k: d[k].numpy() for k in ob.INOUT_KEYS if d[k] is not None}
    got.update({k: v.numpy() for k, v in out.items()})
    assert osc.same(got, osc.expected(a, sh, want)) == []
    assert osc.same({k: v.numpy() for k, v in rout.items()}, {k: ref[k] for k in ("out_desc", "best_obs", "best_median", "status")}) == []
    assert osc.same({k: v.numpy() for k, v in cout.items()}, cov) == []
    assert all(v.intact() for v in list(out.values()) + list(rout.values()) + list(cout.values()) + [v for v in d.values() if v is not None])


def test_chain_culled_keyframes_to_a_second_culling_in_device_memory(matcher):
    """msl_cull_keyframes, its MSL_CULL_CULLED rows as a KF_ERASE log (the caller reads the rows: the decision to send an op is its own),
    then msl_observations_apply and a second msl_cull_keyframes on the tables it leaves, with no copy in between and n_obs_total = ocap.
    The second culling equals cull_model on the scene cull_model's own objects leave after the replay."""
    from manhattanslam_amd import cull, observations as ob
    n_tab, cap = 24, 30
    scene = cs.random_scene(77, n_tab, cap, n_items=1)
    a, sh = cs.pack(scene)
    D = osc.DevArray
    d = {k: D(v) for k, v in a.items()}
    args = lambda n_obs: (cull.cull_params(sh["th_depth"]), n_tab, sh["cap"], sh["n_pts"], 1, n_obs, sh["ccap"], sh["origin"])
    first = cull.cull_keyframes_device(matcher, *args(sh["n_obs_total"]), d, cull.keyframes_outputs(1, sh["ccap"], osc.device_filled))
    matcher.sync()
    status = first["status"].numpy()[0]
    order = [c for c, s_ in zip(scene["items"][0], status) if s_ == cm.CULLED]
    assert order == cm.cull_keyframes(scene, scene["items"][0])[1] and len(order) >= 3
    # what the objects of cull_model leave
    kfs, points = cm.build_objects(scene)
    for c in order:
        kfs[c].set_bad_flag()
    after = dict(scene, held=[[None if m is None else m.id for m in kf.slots] for kf in kfs], pt_bad=[m.bad for m in points],
                 pt_nobs=[m.nobs for m in points], pt_obs=[sorted((kf.k, i) for kf, i in m.obs.items()) for m in points])
    # the observation table of the first culling is in the scene's insertion order: the edits take it ascending
    state = osc.from_cull_scene(scene)
    off, okf, oidx = om.csr(state["obs"])
    entry = dict(obs_off=D(off), obs_kf=D(okf), obs_idx=D(oidx))          # referenced until the stream is drained: the calls are asynchronous
    d.update(entry, pt_ref=D(state["pt_ref"]), ops=D(ob.pack_ops([(om.KF_ERASE, 0, c) for c in order])))
    ocap = sh["n_obs_total"]
    out = ob.outputs(sh["n_pts"], len(order), ocap, sh["n_pts"], osc.device_filled)
    ob.apply_device(matcher, n_tab, sh["cap"], sh["n_pts"], sh["n_obs_total"], len(order), ocap, sh["n_pts"], d, d, out)
    d.update(obs_off=out["obs_off_out"], obs_kf=out["obs_kf_out"], obs_idx=out["obs_idx_out"])
    second = cull.cull_keyframes_device(matcher, *args(ocap), d, cull.keyframes_outputs(1, sh["ccap"], osc.device_filled))
    matcher.sync()
    ops = [(om.KF_ERASE, 0, c) for c in order]
    want = om.apply(dict(state, pt_found=None, pt_visible=None, pt_replaced=None), ops)
    got = {k: d[k].numpy() for k in ("held_id", "pt_flags", "pt_nobs", "pt_ref")}
    got.update({k: v.numpy() for k, v in out.items()})
    e = osc.expected(dict(d, pt_found=None, pt_visible=None, pt_replaced=None), dict(n_pts=sh["n_pts"], n_ops=len(ops), ocap=ocap, tcap=sh["n_pts"]), want)
    assert osc.same(got, e) == [], (got["counts"].tolist(), want["counts"], got["op_status"].tolist(), want["op_status"])
    assert want["counts"][2] == 0 and want["counts"][3] > 0
    assert cs.same({k: v.numpy() for k, v in second.items()}, cs.expected(sh, cs.model(after))) == []
    assert all(v.intact() for v in list(d.values()) + list(entry.values()) + list(out.values()) + list(second.values()))

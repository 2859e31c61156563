"""msl_local_keyframes, msl_local_points and msl_local_lines on the GPU against tests/localmap_model.py: every output, compared as bytes,
in the host-memory forms (the handle's and the device-indexed one) and the device-memory form; every pin of msl.h's list on a hand-built
scene; the output capacity, the group boundary of the scratch budget, the device-memory contract for indices outside their tables with
canaries around every array; and the chain msl_covisibility -> msl_local_keyframes -> msl_local_points -> msl_match_local_points /
msl_local_lines -> msl_match_local_lines on one stream in device memory against the literal models.  The shapes here are small (n_tab up to 130, cap 100, klcap 70, three frames); the limits of msl.h
-- n_tab 4096, cap 8192, klcap 256, mcap 32768, n_pts 1 << 20 -- are in tests/test_mapping_limits_gpu.py."""
import numpy as np
import pytest

from tests import localmap_model as lm
from tests import localmap_scenes as ls

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher():
    from manhattanslam_amd.match import Matcher
    h = Matcher()
    yield h
    h.close()


def check(scene, matcher, mcap=None, mlcap=None, forms=("device", "host"), with_prev=True, **shape):
    """Every output of the three entries equals the model's, in each form; returns the model's results."""
    a, sh = ls.pack(scene, **shape)
    want = ls.model(scene)
    mcap = mcap or max(max(len(w["points"]["local"]) for w in want), 1) + 2
    mlcap = mlcap or max(max(len(w["lines"]["local"]) for w in want), 1) + 2
    e = ls.expected(scene, a, sh, mcap, mlcap, want)
    for form in forms:
        got = ls.run(a, sh, mcap, mlcap, mem=form == "device", handle=None if form == "batch" else matcher, with_prev=with_prev)
        assert ls.same(got, e) == [], form
    return want


@pytest.mark.parametrize("n_tab,cap,frame_sizes", [(3, 5, [4]), (70, 100, [100, 0, 37]), (130, 100, [64]), (130, 5, [5, 3, 0])])
def test_random_graphs_in_every_form(matcher, n_tab, cap, frame_sizes):
    s = ls.random_scene(n_tab + cap, n_tab, cap, n_pts=400, frame_sizes=frame_sizes, klcap=3, lcap=4, n_lines=9)
    check(s, matcher, forms=("device", "host", "batch"), cap=cap)


@pytest.mark.parametrize("klcap", [3, 70])
def test_lines_with_double_rows(matcher, klcap):
    s = ls.random_scene(klcap, 40, 6, n_pts=60, frame_sizes=[6, 2, 5], klcap=klcap, lcap=klcap, n_lines=300)
    want = check(s, matcher, klcap=klcap)
    assert max(len(w["lines"]["local"]) for w in want) > (2 if klcap == 3 else 64)


@pytest.mark.parametrize("first,total", [(78, 83), (80, 82), (81, 81)])
def test_the_stop_above_eighty(matcher, first, total):
    want = check(ls.stop_scene(first), matcher)
    assert len(want[0]["kf"]["local_kf"]) == total                         # exactly 81 pushed by the first loop: the second adds nothing


@pytest.mark.parametrize("walked", [0, 2, 3])
def test_parent_break_at_the_first_a_middle_and_the_last_walked_keyframe(matcher, walked):
    s = ls.vote_scene(12, {0: 1, 1: 1, 2: 1, 3: 1}, conn={k: [4 + k] for k in range(4)}, parent={walked: 11}, kf_bad=(11,))
    want = check(s, matcher)
    assert want[0]["kf"]["local_kf"] == [0, 1, 2, 3] + [4 + k for k in range(walked + 1)] + [11]   # the bad parent is added and ends the walk


def test_neighbours_and_children(matcher):
    # 0: its ten best are all in the list, the eleventh is not looked at; 1: n_conn 0; 2: three neighbours, a bad one in first place;
    # 3: more than ten, the first live one outside the list is the fourth.  Two children of 0 are eligible (the lower wins); 16's parent is
    # the bad keyframe 15, which got votes but is never walked, so 16 does not enter as a child
    voted = {k: 1 for k in range(10)}
    voted[15] = 5
    conn = {0: [1, 2, 3, 4, 5, 6, 7, 8, 9, 1, 12], 2: [13, 3, 14], 3: [0, 1, 2, 13, 17, 18, 4, 5, 6, 7, 8, 9]}
    s = ls.vote_scene(20, voted, conn=conn, parent={10: 0, 11: 0, 16: 15}, kf_bad=(13, 15))
    want = check(s, matcher)[0]["kf"]
    assert want["local_kf"] == list(range(10)) + [10, 14, 17] and want["ref_kf"] == 0 and want["votes"][15] == 5


def test_equal_maxima_one_of_them_bad_and_all_voted_bad(matcher):
    want = check(ls.vote_scene(70, {69: 4, 7: 4, 64: 4, 3: 2}, kf_bad=(7,)), matcher)[0]["kf"]
    assert want["ref_kf"] == 64 and want["local_kf"] == [3, 64, 69]
    want = check(ls.vote_scene(5, {1: 2, 4: 1}, kf_bad=(1, 4)), matcher)[0]["kf"]
    assert want["local_kf"] == [] and want["ref_kf"] is None and want["status"] == 0


def test_no_votes_with_and_without_the_old_list(matcher):
    s = ls.graph(6)
    b, q = ls.add_point(s, [1], bad=True), ls.add_point(s, [])
    s["held"][4] += [q, b]
    s["frames"] += [dict(held=[b, None], lheld=[], prev=[4, 2]), dict(held=[], lheld=[], prev=[5])]
    want = check(s, matcher)
    assert [w["kf"]["status"] for w in want] == [lm.NO_VOTES] * 2 and want[0]["points"]["local"] == [q] and want[0]["kf"]["cleared"] == [0]
    for f in s["frames"]:
        f["prev"] = []
    check(s, matcher, with_prev=False)


def test_points_pins(matcher):
    # p0 sits in two frame slots and in four local keyframes; p1 is bad (in a frame slot and in keyframes); p2 has no observations counted
    # (pt_nobs 0); ids 0 and n_pts - 1 are both local; the frame holds p0, so its mp_flags bit 0 is clear
    s = ls.graph(5)
    p0, p1, p2 = ls.add_point(s, [0, 1, 2, 3]), ls.add_point(s, [0, 2], bad=True), ls.add_point(s, [3, 1], nobs=0)
    rest = [ls.add_point(s, [k % 4]) for k in range(9)]
    s["held"][1] = [None] + s["held"][1]
    s["frames"].append(dict(held=[p0, p1, None, p0, rest[-1]], lheld=[], prev=[]))
    want = check(s, matcher)[0]
    assert want["kf"]["votes"][0] == 3 and want["points"]["local"][0] == p0 and want["points"]["flags"][0] == 2
    assert want["points"]["local"].count(p0) == 1 and p1 not in want["points"]["local"] and rest[-1] in want["points"]["local"]
    assert want["points"]["flags"][want["points"]["local"].index(p2)] == 1 and want["points"]["cur_flags"] == [3, 0, 0, 3, 3]


def test_output_capacity_one_below_at_and_above_the_count(matcher):
    s = ls.random_scene(5, 70, 100, n_pts=400, frame_sizes=[50], klcap=3, lcap=3)
    n = len(ls.model(s)[0]["points"]["local"])
    assert n > 260                                                         # more than one block of slots and of outputs
    for mcap in (n + 1, n, n - 1):
        check(s, matcher, mcap=mcap, forms=("device",), cap=100)


def test_two_groups_of_frames_equal_one(matcher):
    from manhattanslam_amd import localmap
    s = ls.random_scene(11, 70, 100, n_pts=400, frame_sizes=[100, 20, 70], klcap=3, lcap=3, n_lines=50)
    a, sh = ls.pack(s, cap=100)
    one = ls.run(a, sh, 400, 50, mem=1, handle=matcher)
    localmap.set_budget(matcher, 2 * 4 * sh["n_pts"])                      # two frames of point stamps, and more than three of line stamps
    try:
        two = ls.run(a, sh, 400, 50, mem=1, handle=matcher)
        localmap.set_budget(matcher, 4)                                    # one frame at a time
        three = ls.run(a, sh, 400, 50, mem=1, handle=matcher)
    finally:
        localmap.set_budget(matcher)
    e = ls.expected(s, a, sh, 400, 50)
    assert ls.same(one, e) == [] and ls.same(two, e) == [] and ls.same(three, e) == []


def test_indices_outside_their_tables_are_absent_and_nothing_is_written_outside(matcher):
    """The device-memory contract: out-of-table ids, keyframes, neighbours, parents and counts beyond their capacity give the result of the
    scene without them, and the canaries around every input and output stay."""
    n_tab, cap = 70, 100
    s = ls.random_scene(23, n_tab, cap, n_pts=300, frame_sizes=[cap, 31], klcap=3, lcap=3, n_lines=9)
    s["held"][5] = (s["held"][5] + [None] * cap)[:cap]
    bad = [k for k in range(n_tab) if s["kf_bad"][k]]
    assert bad
    for k in range(0, n_tab, 3):                                           # a bad keyframe in the list is as good as none: replaced below
        s["conn"][k] = [bad[0]] + [c for c in s["conn"][k] if c != bad[0]]
    s["conn"][1] = (s["conn"][1] + [c for c in range(n_tab) if c != 1 and c not in s["conn"][1]])[:n_tab - 1]
    s["frames"].append(dict(held=[], lheld=[], prev=[3, 9]))               # no votes: the old list is copied as it stands
    a, sh = ls.pack(s, cap=cap, ccap=n_tab - 1)
    e = ls.expected(s, a, sh, 300, 9)
    a["held_id"][a["held_id"] == -1] = np.resize([sh["n_pts"], -7, 1 << 30], (a["held_id"] == -1).sum())
    a["cur_held"][a["cur_held"] == -1] = np.resize([sh["n_pts"], -5, 1 << 30], (a["cur_held"] == -1).sum())
    a["lheld_id"][a["lheld_id"] == -1] = sh["n_lines"]
    a["cur_lheld"][a["cur_lheld"] == -1] = -3
    a["conn"][a["conn"] == bad[0]] = np.resize([n_tab, -2], (a["conn"] == bad[0]).sum())
    a["parent"][a["parent"] == -1] = np.resize([n_tab + 5, -9], (a["parent"] == -1).sum())
    a["n_cur"][0] = cap + 7; a["n_kps"][5] = cap + 1; a["n_conn"][1] = n_tab + 3   # full rows: the clamp changes nothing
    a["prev_kf"][2, 2:4] = [n_tab, -1]; a["n_prev"][2] = 4                 # copied as they stand; msl_local_points finds no such keyframe
    e["local_kf"][2, 2:4] = [n_tab, -1]; e["n_local_kf"][2] = 4
    keep = {}
    got = ls.run(a, sh, 300, 9, mem=1, handle=matcher, keep=keep)
    assert ls.same(got, e) == []
    assert [k for k, v in keep.items() if v is not None and not v.intact()] == []


def test_chain_on_one_stream_in_device_memory(matcher):
    """msl_covisibility -> msl_local_keyframes -> msl_local_points -> msl_match_local_points and msl_local_lines -> msl_match_local_lines
    with nothing read back in between; the matches equal localmap_model into local_match_model / line_match_model."""
    from manhattanslam_amd import LINE_TRACK_DTYPE, localmap, mappoint, match  # noqa: F401
    from tests import line_match_model as lnm, line_match_scenes as lns, local_match_model as lmm, local_match_scenes as lms, mappoint_model as mm
    n_tab, cap, n_pts, lcap, n_lines, th = 12, 80, 240, 20, 60, 3
    p, lp = lms.params(), lns.params(th=1.0)
    cur, local, T = lms.random_frame(3, p, n_cur=cap, n_local=n_pts, preheld=0)
    lcur, llocal, _ = lns.local_frame(3, lp, n_kl=lcap, n_local=n_lines, preheld=0, T=T)
    s = ls.random_scene(31, n_tab, cap, n_pts, frame_sizes=[cap], klcap=lcap, lcap=lcap, n_lines=n_lines, bad=0.05)
    rng = np.random.default_rng(2)
    s["frames"][0]["held"] = [None if rng.random() < 0.6 else int(rng.integers(0, n_pts)) for _ in range(cap)]
    s["frames"][0]["lheld"] = [None if rng.random() < 0.6 else int(rng.integers(0, n_lines)) for _ in range(lcap)]
    a, sh = ls.pack(s, cap=cap, klcap=lcap, lcap=lcap, ccap=n_tab)
    for k in ("xyz", "normal", "dist", "desc"):
        a["pt_" + k], a["ln_" + k] = np.ascontiguousarray(local[k]), np.ascontiguousarray(llocal[k])
    # the model: UpdateConnections' lists, then UpdateLocalMap and the two searches
    obs = [[(k, 0) for k in o] for o in s["pt_obs"]]
    cv = mm.covisibility([dict(held_id=r) for r in a["held_id"]], obs, a["pt_flags"], list(range(n_tab)), th=th, ccap=n_tab)
    s["conn"] = [[int(c) for c in cv["conn"][k, :cv["n_conn"][k]]] for k in range(n_tab)]
    w = lm.update_local_map(s, s["frames"][0])
    assert len(w["kf"]["local_kf"]) > 3 and len(w["points"]["local"]) > 60 and len(w["lines"]["local"]) > 10
    rows = lambda t, r: dict({k: a[t + "_" + k][r["local"]] for k in ("xyz", "normal", "dist", "desc")}, flags=np.array(r["flags"], np.uint8))
    want_p = lmm.search_local_points(p, dict(cur, flags=np.array(w["points"]["cur_flags"], np.uint8)), rows("pt", w["points"]), T)
    want_l = lnm.search_local_lines(lp, dict(lcur, flags=np.array(w["lines"]["cur_flags"], np.uint8)), rows("ln", w["lines"]), T)
    assert want_p[2] > 5 and want_l[2] > 0
    # the device: everything stays there
    D = ls.DevArray
    d = {k: D(v) for k, v in a.items()}
    covis = {k: D(v) for k, v in mappoint.covisibility_outputs(n_tab, n_tab, n_tab).items()}
    mappoint.covisibility_device(matcher, n_tab, cap, n_pts, n_tab, sh["n_obs_total"], n_tab, th, d["held_id"], d["n_kps"], d["pt_flags"], d["obs_off"],
                                 d["obs_kf"], D(np.arange(n_tab, dtype=np.int32)), covis)
    d["conn"], d["n_conn"] = covis["conn"], covis["n_conn"]
    kf = localmap.local_keyframes_device(matcher, 1, cap, n_tab, n_pts, sh["n_obs_total"], n_tab, d, localmap.keyframes_outputs(1, cap, n_tab, ls.device_filled))
    d["local_kf"], d["n_local_kf"] = kf["local_kf"], kf["n_local_kf"]
    pts = localmap.local_points_device(matcher, 1, n_tab, cap, n_pts, n_pts, d, localmap.points_outputs(1, cap, n_pts, ls.device_filled))
    lns_out = localmap.local_lines_device(matcher, 1, n_tab, lcap, lcap, n_lines, n_lines, d, localmap.lines_outputs(1, lcap, n_lines, ls.device_filled))
    _, _, pa = match.pack_local_points([dict(cur, flags=np.zeros(cap, np.uint8))], [lms.empty_local(local)], T[None], cap, n_pts)
    _, _, la = match.pack_local_lines([dict(lcur, flags=np.zeros(lcap, np.uint8))], [lns.empty(llocal)], T[None], lcap, n_lines)
    mo, ntm, nm = ls.device_filled((1, cap), np.int32), ls.device_filled((1,), np.int32), ls.device_filled((1,), np.int32)
    matcher.search_local_points_device(p, 1, cap, n_pts, [D(x) for x in pa[:6]] + [pts[k] for k in ("cur_flags", "mp_xyz", "mp_normal", "mp_dist", "mp_desc",
                                                                                                  "mp_flags", "n_local")] + [D(pa[-1])], mo, ntm, nm)
    lmo, lntm, lnmm = ls.device_filled((1, lcap), np.int32), ls.device_filled((1,), np.int32), ls.device_filled((1,), np.int32)
    matcher.search_local_lines_device(lp, 1, lcap, n_lines, [D(x) for x in la[:3]] + [lns_out[k] for k in ("cur_line_flags", "ml_xyz", "ml_normal", "ml_dist",
                                                                                                          "ml_desc", "ml_flags", "n_local_lines")] + [D(la[-1])],
                                      lmo, lntm, lnmm)
    matcher.sync()
    assert np.array_equal(covis["conn"].numpy(), cv["conn"]) and np.array_equal(pts["local_id"].numpy()[0, :len(w["points"]["local"])], w["points"]["local"])
    assert np.array_equal(mo.numpy()[0], want_p[0]) and (int(ntm.numpy()[0]), int(nm.numpy()[0])) == (want_p[1], want_p[2])
    assert np.array_equal(lmo.numpy()[0], want_l[0]) and (int(lntm.numpy()[0]), int(lnmm.numpy()[0])) == (want_l[1], want_l[2])

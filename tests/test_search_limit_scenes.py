"""The scenes of tests/search_limit_scenes.py reach what they are there for: asserted without a GPU from each case's facts, from the packed
arrays and from the traces of the sequential models.  The searching cases also keep the margin rule of tests/test_fuse_model.py::
test_margins -- no float comparison within 1e-3 (relative to its threshold's scale) of its threshold -- with at most 5 % of their live
candidates retired to get there."""
import numpy as np

from tests import fuse_model as fm
from tests import linefuse_model as lf
from tests import mappoint_model as mm
from tests import search_limit_scenes as S

N = S.MAX_PTS


def _beyond_margin(margins):
    assert len(margins) > 100
    for what, lhs, rhs, scale in margins:
        assert abs(lhs - rhs) > S.MARGIN * abs(scale), (what, lhs, rhs, scale)


# ---- msl_fuse_candidates ---------------------------------------------------------------------------------------------------------------
def test_c1_reaches():
    c = S.c1()
    f, sh, cand, n_cand = c["facts"], c["sh"], c["e"]["cand"], c["e"]["n_cand"]
    assert (sh["tcap"], sh["cap"], sh["lcap"], sh["n_pts"]) == (64, 8192, 65536, N) and sh["n_tab"] >= 65
    item0, item1 = c["items"]
    assert len(item0) == 64 and len(set(item0)) == 63                           # a target named twice
    assert n_cand[0] > 65536 and (cand[0] >= 0).all() and len(set(cand[0].tolist())) == 65536   # exactly lcap distinct ids are written
    held = c["a"]["held_id"]
    assert held[item0[0], 8191] == f["both"] == held[item0[63], 0]              # rank 0 slot 8191 and rank 63 slot 0: the first wins
    full = fm.fuse_candidates([dict(held_id=h) for h in held], dict(flags=c["a"]["pt_flags"]), [item0])[0][0]
    assert full.count(f["both"]) == 1 and full.index(f["both"]) < 8192 and len(full) == n_cand[0]
    assert (held[item0[0]] == f["twice"]).sum() == 2 and full.count(f["twice"]) == 1
    assert f["bad_held"] in held[item0[0]] and not c["a"]["pt_flags"][f["bad_held"]] and f["bad_held"] not in full
    assert {0, N - 1} <= set(cand[0, :8192].tolist())
    assert n_cand[1] == 65535 and cand[1, 65534] >= 0 and cand[1, 65535] == -1  # the -1 fill is one entry


def test_c2_reaches():
    c = S.c2()
    sh, want = c["sh"], c["want"]
    assert sh["n_pts"] == N and sh["n_items"] == 40 and c["facts"]["per_launch"] == S.CAND_SCRATCH // N == 16
    for f in range(16):
        first = {p: i for i, p in enumerate(want[f][0])}
        assert {0, N - 1} <= set(first)
        for g in (f + 16, f + 32)[:2 if f < 8 else 1]:                          # the same ids at a larger position in the later launch
            later = {p: i for i, p in enumerate(want[g][0])}
            assert set(first) <= set(later) and c["items"][g][-1] == f
            assert all(later[p] >= first[p] for p in first) and later[0] > first[0] and later[N - 1] > first[N - 1]
            assert int(c["e"]["n_cand"][g]) == len(later) > len(first)


def test_c3_reaches():
    c = S.c3()
    assert c["sh"]["n_items"] == 4096 and 4096 % c["facts"]["period"] and len(c["items"]) == c["facts"]["period"]
    assert (c["e"]["n_cand"] > c["sh"]["lcap"]).any() and (c["e"]["n_cand"] == 0).any()
    assert c["a"]["targets"][4095].tolist() == c["a"]["targets"][4095 % 37].tolist() != c["a"]["targets"][0].tolist()


# ---- msl_covisibility ------------------------------------------------------------------------------------------------------------------
def test_v1_reaches():
    c = S.v1()
    f, sh, e = c["facts"], c["sh"], c["e"]
    assert (sh["n_tab"], sh["cap"], sh["ccap"]) == (4096, 8192, 4096)
    k0 = f["item"]
    assert c["a"]["n_kps"][k0] == 8192 and c["a"]["pt_flags"][c["a"]["held_id"][k0]].all() and len(set(c["a"]["held_id"][k0].tolist())) == 8192
    assert np.array_equal(e["weight"][0], f["weights"]) and e["weight"][0, f["full"]] == 8192 and e["weight"][0, k0] == 0
    assert (np.delete(e["weight"][0], k0) >= sh["th"]).all() and e["n_conn"][0] == 4095
    conn, w = e["conn"][0, :4095], e["conn_w"][0, :4095]
    assert (conn[0], w[0]) == (f["full"], 8192) and 4095 in conn and e["conn"][0, 4095] == -1
    same = w[1:] == w[:-1]
    assert same.sum() > 4000 and (conn[1:][same] < conn[:-1][same]).all() and (w[1:] <= w[:-1]).all()   # equal weights by descending index


def test_v2_reaches():
    c = S.v2()
    f, sh, e = c["facts"], c["sh"], c["e"]
    assert sh["n_items"] == sh["n_tab"] == 4096 and e["weight"].shape == (4096, 4096) and 4096 % f["period"]
    assert c["a"]["kf"].tolist() == list(range(4096))
    for i, k in enumerate(f["own"]):                                            # they observe their own points and do not count themselves
        assert e["weight"][k, k] == 0 and e["n_conn"][k] > 0 and np.array_equal(e["weight"][k], f["small"]["weight"][f["period"] + i])
    assert 4095 in f["own"] and (e["n_conn"] > sh["ccap"]).any() and (e["n_conn"] == 0).any()
    assert (e["weight"][np.arange(4096), np.arange(4096)] == 0).all()


# ---- msl_refresh_map_points / msl_refresh_map_lines ------------------------------------------------------------------------------------
def _refresh_reaches(c, n_tab, cap):
    f, sh, a, e = c["facts"], c["sh"], c["a"], c["e"]
    assert (sh["n_pts"], sh["n_tab"], sh["cap"]) == (N, n_tab, cap)
    assert {0, N - 1} <= set(f["named"].tolist())
    assert (a["obs_kf"] == n_tab - 1).any() and (a["obs_idx"] == cap - 1).any()
    assert a["pt_ref"][N - 1] == n_tab - 1 and (n_tab - 1, cap - 1) in f["obs"][N - 1]      # the reference keyframe and its index
    assert a["obs_off"][N - 1] < a["obs_off"][N] == sh["n_obs_total"]                       # a range ending at n_obs_total
    st = dict(zip(f["named"].tolist(), f["want"]["status"].tolist()))
    assert st[0] == st[N - 1] == mm.DESC_WRITTEN | mm.NORMAL_WRITTEN
    assert all(st[int(p)] == mm.BAD for p in f["dead"]) and all(st[int(p)] == mm.NO_OBS for p in f["empty"]) and len(f["dead"]) > 10
    return st


def _rows_keep_sentinel(c, keys, ids):
    """Only the rows of ids differ from the sentinel."""
    for k in keys:
        changed = np.flatnonzero((c["e"][k].view(np.uint8).reshape(N, -1) != S.FILL).any(1))
        assert 1000 < len(changed) and set(changed.tolist()) <= set(int(p) for p in ids)


def test_r1_reaches():
    c = S.r1()
    st = _refresh_reaches(c, 4096, 128)
    p256, p257 = c["facts"]["many"]
    live = lambda p: sum(1 for k, _ in c["facts"]["obs"][p] if k != 3)
    assert (live(p256), live(p257)) == (256, 257) and st[p256] & mm.DESC_WRITTEN and st[p257] & mm.TOO_MANY and not st[p257] & mm.DESC_WRITTEN
    _rows_keep_sentinel(c, ("pt_desc", "pt_normal", "pt_dist"), c["facts"]["named"])


def test_r1c_reaches():
    c = S.r1c()
    _refresh_reaches(c, 8, 8192)
    _rows_keep_sentinel(c, ("pt_desc", "pt_normal", "pt_dist"), c["facts"]["named"])


def test_r2_reaches():
    c = S.r2()
    _refresh_reaches(c, 40, 64)
    sh, e = c["sh"], c["e"]
    assert sh["n_items"] == N and sorted(c["a"]["ids"].tolist()) == list(range(N))
    real = e["status"] != mm.BAD
    assert 2900 < real.sum() < 3100 and (e["best_obs"][~real] == -1).all() and not e["out_desc"][~real].any()
    assert np.array_equal(np.sort(c["a"]["ids"][real]), np.sort(c["facts"]["named"][c["facts"]["want"]["status"] != mm.BAD]))


def test_r3_reaches():
    c = S.r3()
    f, sh, a, e = c["facts"], c["sh"], c["a"], c["e"]
    assert (sh["n_lines"], sh["klcap"], sh["n_tab"]) == (N, 256, 4096)
    st = dict(zip(a["ids"].tolist(), e["status"].tolist()))
    assert st[0] == st[N - 1] == lf.NORMAL_WRITTEN
    assert (a["obs_kf"] == 4095).any() and (a["obs_idx"] == 255).any() and a["ln_ref"][N - 1] == 4095 and (4095, 255) in f["obs"][N - 1]
    assert a["obs_off"][N - 1] < a["obs_off"][N] == sh["n_obs_total"]
    assert all(st[int(p)] == lf.R_BAD for p in f["dead"]) and all(st[int(p)] == lf.NO_OBS for p in f["empty"])
    _rows_keep_sentinel(c, ("ln_normal", "ln_dist"), a["ids"])


# ---- msl_fuse_map_points ---------------------------------------------------------------------------------------------------------------
def _retired_within_cap(f):
    assert len(f["retired"]) <= S.RETIRED_CAP * f["n_live"], (len(f["retired"]), f["n_live"])
    print("retired", len(f["retired"]), "of", f["n_live"])


def test_p1_reaches():
    c = S.p1()
    f, sh, res, lst, kf = c["facts"], c["sh"], c["res"][0], c["lst"], c["kf"]
    assert (sh["cap"], sh["lcap"], sh["n_pts"]) == (8192, 65536, N) and len(lst) == 65536 and len(kf["kps_un"]) == 8192
    st, bi = res["status"], res["best_idx"]
    at = {p: j for j, p in enumerate(lst) if p >= 0}
    assert len(at) == sum(1 for p in lst if p >= 0)                             # distinct ids
    assert not set(f["retired"]) & set(f["placed"])
    searched = st >= fm.BEHIND
    assert 3500 < searched.sum() < 4500 and 1500 < (kf["held_id"] >= 0).sum() < 2600
    assert all(st[at[p]] >= fm.BEHIND for p in f["ends"])                       # ids 0 and 1048575 reach the search
    assert set(st.tolist()) == set(range(15))                                   # every status: the scene can produce them all
    j1, j2, j3 = (at[p] for p in f["hits"])
    assert (j1, j2, j3) == (40000, 50000, 65535) and bi[j1] == bi[j2] == bi[j3] == f["top"] == 8191       # a winner at slot 8191
    assert not ((bi == 8191) & (np.arange(65536) < j1)).any()                   # so j2 >= 32768 is the second hit of its slot
    assert st[j1] == fm.ADDED and st[j2] in (fm.REPLACED_BY_HELD, fm.REPLACES_HELD) and st[j3] == fm.UNRESOLVED   # and j = 65535 the third
    cell = kf["grid_cell"]
    order = np.lexsort((np.arange(8192), cell))
    order = order[cell[order] >= 0]
    pos = np.empty(8192, np.int64); pos[order] = np.arange(len(order))
    won = pos[bi[st >= fm.ADDED]]
    assert (won > 4096).sum() > 500 and (won > 8000).any()
    ties = [t for tr in res["trace"] if tr for t in tr.get("ties", []) if t[2] != t[3]]
    assert ties and {f["A"], f["B"]} == set(res["trace"][at[f["twin"]]]["ties"][0][:2]) and st[at[f["twin"]]] >= fm.ABOVE_TH_LOW
    assert max(tr["cells"] for tr in res["trace"] if tr and "cells" in tr) > 64
    held = set(int(h) for h in kf["held_id"] if h >= 0)
    assert min(held) == f["held_min"] and max(held) == f["held_max"] and st[at[f["held_min"]]] == st[at[f["held_max"]]] == fm.IN_KEYFRAME
    m = f["mid"]
    assert m in held and st[at[m]] == fm.IN_KEYFRAME and m - 1 not in held and m + 1 not in held
    assert st[at[m - 1]] >= fm.BEHIND and st[at[m + 1]] >= fm.BEHIND            # one below and one above a held id: not held
    assert all(st[at[p]] == fm.NO_FEATURE for p in f["hole"])
    _retired_within_cap(f)
    _beyond_margin(S.fuse_margins(c["prm"], kf, c["pts"], lst))


def test_p2_reaches():
    c = S.p2()
    f, sh, a = c["facts"], c["sh"], c["a"]
    assert sh["n_items"] == sh["n_tab"] == sh["n_lists"] == 4096 and 4096 % f["period"] and 8 <= sh["cap"] <= 16 and 8 <= sh["lcap"] <= 16
    assert (a["tgt"][4095], a["list"][4095]) == (4095, 4095) and a["list"][4] == a["list"][5] == 4
    assert {fm.ADDED, fm.REPLACED_BY_HELD, fm.REPLACES_HELD, fm.UNRESOLVED, fm.IN_KEYFRAME} <= set(x for r in c["res"] for x in r["status"].tolist())
    assert c["e"]["status"][5].tobytes() != c["e"]["status"][5 + f["period"]].tobytes()
    _retired_within_cap(f)
    m = []
    for t, l in f["pairs"]:
        m += S.fuse_margins(c["prm"], c["kfs"][t], c["pts"], c["lists"][l])
    _beyond_margin(m)


# ---- msl_fuse_map_lines ----------------------------------------------------------------------------------------------------------------
def test_l1_reaches():
    c = S.l1()
    f, sh, res, lst, kf = c["facts"], c["sh"], c["res"][0], c["lst"], c["kf"]
    assert (sh["klcap"], sh["lcap"], sh["n_lines"]) == (256, 65536, N) and len(lst) == 65536 and len(kf["kl"]) == 256
    st, bi = res["status"], res["best_idx"]
    at = {p: j for j, p in enumerate(lst) if p >= 0}
    assert len(at) == sum(1 for p in lst if p >= 0) and not set(f["retired"]) & set(f["placed"])
    assert 2000 < (st >= lf.BEHIND).sum() < 5000
    assert set(st.tolist()) == set(range(15))                                   # every status: the scene can produce them all
    assert all(st[at[p]] >= lf.ADDED for p in f["ends"])                        # ids 0 and 1048575 are matched
    j1, j2, j3 = (at[p] for p in f["hits"])
    assert (j1, j2, j3) == (40000, 50000, 65535) and bi[j1] == bi[j2] == bi[j3] == f["top"] == 255        # a winner at keyline 255
    assert not (bi[:j1] == 255).any()                                           # so the first and the second hit are at j >= 32768
    assert st[j1] == lf.ADDED and st[j2] in (lf.REPLACED_BY_HELD, lf.REPLACES_HELD) and st[j3] == lf.UNRESOLVED
    js = [at[f["own"]]] + [at[p] for p in f["after_self"]]
    assert js == sorted(js) and all(bi[j] == f["self_kl"] for j in js) and not (bi[:js[0]] == f["self_kl"]).any()
    assert st[js[0]] == lf.SELF and st[js[1]] in (lf.REPLACED_BY_HELD, lf.REPLACES_HELD) and st[js[2]] == lf.UNRESOLVED   # UNRESOLVED after SELF
    j = at[f["twice"]]
    assert kf["held_id"][f["elsewhere"]] == f["twice"] and kf["held_id"][f["empty_kl"]] == -1
    assert (bi[j], st[j]) == (f["empty_kl"], lf.ADDED) and res["added_in_kf"] >= 1 and not (bi[:j] == f["empty_kl"]).any()
    _retired_within_cap(f)
    _beyond_margin(S.line_margins(c["prm"], kf, c["lines"], lst))


def test_l2_reaches():
    c = S.l2()
    f, sh, a = c["facts"], c["sh"], c["a"]
    assert sh["n_items"] == sh["n_tab"] == sh["n_lists"] == 4096 and 4096 % f["period"]
    assert (a["tgt"][4095], a["list"][4095]) == (4095, 4095) and a["list"][4] == a["list"][5] == 4
    assert {lf.ADDED, lf.REPLACED_BY_HELD, lf.REPLACES_HELD, lf.UNRESOLVED, lf.SELF} <= set(x for r in c["res"] for x in r["status"].tolist())
    _retired_within_cap(f)
    m = []
    for t, l in f["pairs"]:
        m += S.line_margins(c["prm"], c["kfs"][t], c["lines"], c["lists"][l])
    _beyond_margin(m)


# ---- msl_triangulate_new_points --------------------------------------------------------------------------------------------------------
def _margins_without_retiring(c):
    """The triangulation scenes keep the margin rule by their seeds alone: nothing is retired."""
    assert c["facts"]["retired"] == []
    _retired_within_cap(c["facts"])
    _beyond_margin(c["margins"])


def test_t1_reaches():
    from tests import triangulate_model as tm
    c = S.t1()
    f, sh, res, table = c["facts"], c["sh"], c["res"][0], c["table"]
    cur, nb = c["items"][0]
    assert (sh["n_tab"], sh["ncap"]) == (4096, 16) and sh["cap"] <= 256 and c["prm"]["check_orientation"]
    assert cur == 4095 and len(nb) == 16 and {0, 4094} <= set(nb) and len(set(nb)) == 16
    assert [k for k, kf in enumerate(table) if len(kf["kps_un"])] == sorted([cur] + nb)        # every other keyframe has n_kps = 0
    skipped = [r for r, tr in enumerate(res["trace"]) if tr["skipped"]]
    assert skipped == [f["skipped"]] == [8] and (res["status"][8] == tm.NEIGHBOUR_SKIPPED).all()
    assert (res["new_neigh"] == 0).sum() >= 8 and (res["new_neigh"] == 15).sum() >= 4           # points created by ranks 0 and 15
    assert len(set(res["new_neigh"].tolist()) - {-1}) >= 10
    # taken at rank 0 and still a candidate at rank 12: the function that forgets the mask matches it there, the entry gives -1
    loose = tm.create_new_map_points(c["prm"], table, cur, nb, use_mask=False)
    again = [i for i in np.flatnonzero(res["new_neigh"] == 0) if loose["match12"][12, i] >= 0]
    assert len(again) >= 3 and all(res["match12"][12, i] == -1 for i in again)
    assert all(table[cur]["tags"][i] in table[nb[12]]["tags"] for i in again)
    _margins_without_retiring(c)


def test_t2_reaches():
    from tests import triangulate_model as tm
    c = S.t2()
    f, sh, a = c["facts"], c["sh"], c["a"]
    assert (sh["n_items"], sh["cap"], sh["ncap"]) == (65535, 8, 2) and 65535 % f["period"] and len(c["items"]) == f["period"]
    assert a["cur"][65534] == c["items"][65534 % 37][0] != a["cur"][0] and c["e"]["n_new"][65534] == len(c["res"][65534 % 37]["new_order"])
    assert {1, 2} == set(a["n_neigh"].tolist()) and max(len(k["kps_un"]) for k in c["table"]) == 8
    seen = set(x for r in c["res"] for x in r["status"].ravel().tolist())
    assert {tm.TRIANGULATED, tm.NEIGHBOUR_SKIPPED, tm.NO_MATCH} <= seen and sum(len(r["new_order"]) for r in c["res"]) > 100
    _margins_without_retiring(c)

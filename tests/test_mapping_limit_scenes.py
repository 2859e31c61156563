"""The scenes of tests/mapping_limit_scenes.py on the sequential models, without a GPU: each scene reaches the edge it was built for, named
after the loop or layout of msl_local_map.hip / msl_cull.hip that it is there for, and the second, literal models agree where the scene is
small enough for them.  tests/test_mapping_limits_gpu.py runs the entries on the same scenes."""
import numpy as np
import pytest

from tests import cull_model as cm
from tests import cull_scenes as cs
from tests import localmap_model as lm
from tests import localmap_scenes as ls
from tests import mapping_limit_scenes as ms

LKF_NT, LM_NT, WAVE = ms.LKF_NT, ms.LM_NT, ms.WAVE


def _kept(name, f=0, lines=False):
    s, w = ms.case(name)[0], ms.want(name)[f]
    kept = ms.kept_slots(w["kf"]["local_kf"], s["lheld" if lines else "held"], s["ln_bad" if lines else "pt_bad"])
    table = s["lheld" if lines else "held"]
    flat = [table[k][i] for k, row in zip(w["kf"]["local_kf"], kept) for i in row]
    assert flat == w["lines" if lines else "points"]["local"]              # kept_slots restates update_local_elements
    return kept


# ---- a to c: k_local_kf ------------------------------------------------------------------------------------------------------------------
def test_a_every_keyframe_voted():
    s, facts = ms.case("a")
    w = ms.want("a")
    n = facts["n_tab"]
    assert n == 4096 and max(len(f["held"]) for f in s["frames"]) == facts["cap"]
    # the j += LKF_NT loops (LDS initialisation, vote write-out) make four rounds; the first loop's compaction fills all 64 chunks
    assert [w[0]["kf"]["votes"][k] for k in range(n)] == facts["votes0"] and len(w[0]["kf"]["votes"]) == n > 3 * LKF_NT
    # s_list holds every index up to 4095; the list is longer than 80, so the second loop stops at once
    assert w[0]["kf"]["local_kf"] == facts["lists"][0] and w[1]["kf"]["local_kf"] == facts["lists"][1]
    # wave_max / wave_min: the lowest index among 4096 equal maxima, then a single maximum in the last lane of the last chunk
    assert [x["kf"]["ref_kf"] for x in w] == facts["ref"] and w[1]["kf"]["votes"][n - 1] == 7 == 1 + w[1]["kf"]["votes"][0]
    # keyframeCounter.empty(): a prev_kf row of n_tab entries is copied as it stands
    assert w[2]["kf"]["status"] == lm.NO_VOTES and w[2]["kf"]["local_kf"] == facts["lists"][2] and sorted(facts["lists"][2]) == list(range(n))
    for f in range(3):
        assert lm.first_occurrence_scan(w[f]["kf"]["local_kf"], s["held"], s["pt_bad"]) == w[f]["points"]["local"]


def test_b_walk_over_the_whole_table():
    s, facts = ms.case("b")
    w = [x["kf"] for x in ms.want("b")]
    n, voted = facts["n_tab"], facts["voted"]
    assert n == 4096 and 65 <= len(voted) <= 75 and voted[0] == 0 and voted[-1] == n - 1
    assert len(s["conn"][0]) == facts["ccap"] == n and len(s["conn"][facts["childless"]]) == 11     # n_conn = ccap, and one above ten
    # frame 0: 4095 gets a vote and enters s_list in the first loop; nothing stops the walk before its 11th addition
    assert w[0]["local_kf"][:len(voted)] == voted and len(voted) <= lm.LOCAL_KF_STOP
    assert len(w[0]["local_kf"]) == lm.LOCAL_KF_STOP + 1                   # the stop above eighty triggers late in the walk, not at once
    for f in range(3):
        # the neighbour read at row stride ccap = 4096: keyframe 0's tenth neighbour, an index above 4032
        # (in frame 2 the first of the ten, 68, has no vote and is taken instead)
        assert (facts["neighbour"] if f < 2 else facts["childless"]) in w[f]["local_kf"][len(w[f]["votes"]):] and facts["neighbour"] > n - WAVE
        # the child search: 1000 (chunk 15) is bad, 2081 (chunk 32) is listed, 2085 (chunk 32) is taken and 3000 is not
        assert facts["middle_child"] in w[f]["local_kf"] and facts["later_child"] not in w[f]["local_kf"]
        assert facts["middle_child"] // WAVE == 32 == facts["skipped_children"][1] // WAVE and facts["skipped_children"][0] not in w[f]["local_kf"]
        assert facts["eleventh"] not in w[f]["local_kf"]                   # the eleventh neighbour is never looked at
    # frame 0: keyframe 68 is walked and its only child, 4095, is listed: every chunk of the child search runs and finds nothing
    assert facts["childless"] in voted and w[0]["local_kf"].count(facts["top"]) == 1
    # frame 1: 4095 has no vote and is found as a child in chunk 63, lane 63
    n1 = len(voted) - 1
    assert w[1]["votes"].get(facts["top"]) is None and facts["top"] in w[1]["local_kf"][n1:] and facts["top"] // WAVE == 63
    # frame 2: a parent at index 4095 (int16_t s_parent) is pushed and ends the walk; the keyframes after 129 add nothing
    assert w[2]["local_kf"][-1] == facts["top"] and s["parent"][129] == facts["top"] and len(w[2]["local_kf"]) < lm.LOCAL_KF_STOP
    assert 4042 in w[0]["local_kf"] and 4042 not in w[2]["local_kf"]


def test_c_full_frame():
    s, facts = ms.case("c")
    w = [x["kf"] for x in ms.want("c")]
    assert [len(f["held"]) for f in s["frames"]] == facts["n_cur"] == [8192, 1025, 1024]
    # the slot loop of k_local_kf: eight rounds, then one thread in a second round, then exactly one round
    assert [x["cleared"] for x in w] == facts["cleared"] and max(facts["cleared"][0]) == 8191 and min(facts["cleared"][0]) >= LKF_NT
    # s_cnt counts per observation: more votes than the frame has slots
    assert w[0]["votes"][facts["voted"]] >= 8192 and w[0]["ref_kf"] == facts["voted"]
    assert 4 in w[0]["votes"] and 4 not in w[0]["local_kf"]                # a bad keyframe keeps its votes and stays out of the list


# ---- d to h: the k_lm_* compaction -------------------------------------------------------------------------------------------------------
def test_d_full_keyframe():
    s, facts = ms.case("d")
    w = ms.want("d")[0]
    assert w["kf"]["local_kf"] == [0, 1, 2, 3, 4] and [len(h) for h in s["held"]] == facts["n_kps"] == [257, 8192, 256, 0, 300]
    kept = _kept("d")
    full = kept[facts["full"]]
    chunks = {i // LM_NT for i in full}
    # k_lm_write carries base through all 32 chunks of one keyframe; one chunk in the middle adds nothing to it
    assert chunks == set(range(32)) - {facts["empty_chunk"]} and full[0] == 0 and full[-1] == 8191
    assert len(kept[0]) > 0 and kept[0][-1] <= LM_NT and len(kept[2]) > 0 and kept[3] == [] and len(kept[4]) > 0
    # ids recur: a later keyframe holds live ids that an earlier one keeps
    earlier = {s["held"][1][i] for i in full} | {s["held"][0][i] for i in kept[0]}
    assert len([p for p in s["held"][2] + s["held"][4] if p in earlier]) > 50
    # the cut j >= D.mcap inside the sixth chunk of the full row: kept slots of that chunk on both sides of it
    cut = ms.mcap_cut()
    assert any(5 * LM_NT <= i < facts["cut_slot"] for i in full) and any(facts["cut_slot"] <= i < 6 * LM_NT for i in full)
    assert len(kept[0]) + LM_NT < cut < len(w["points"]["local"]) - LM_NT < ms.MAX_MCAP
    # k_lm_held runs 32 blocks; the last holds live, bad, NULL and repeated ids
    cur = s["frames"][0]["held"]
    b, e = facts["last_block"]
    assert len(cur) == 8192 and w["points"]["cur_flags"][b:b + 5] == [w["points"]["cur_flags"][b], 0, 0] + [w["points"]["cur_flags"][b + 3]] * 2
    assert w["points"]["cur_flags"][b] & 1 and w["points"]["cur_flags"][b + 3] & 1 and w["points"]["cur_flags"][e - 1] & 1 and cur[b + 2] is None
    assert 0 in [fl & 1 for fl in w["points"]["flags"]] and 1 in [fl & 1 for fl in w["points"]["flags"]]


def test_e_full_list():
    s, facts = ms.case("e")
    w = ms.want("e")[0]
    order = w["kf"]["local_kf"]
    assert len(order) == 4096 == facts["n_tab"] and w["kf"]["status"] == lm.NO_VOTES
    kept = _kept("e")
    counts = [len(r) for r in kept]
    # k_lm_scan: block_scan_array_incl makes sixteen passes per thread over 4096 counts, zeros among them
    assert 0 in counts and max(counts) >= 3 and sum(counts) == len(w["points"]["local"]) > 1000
    for pos in facts["scan_positions"]:                                    # the exclusive scan at 255, 256, 257 and 4095
        assert counts[pos] >= 1 and w["points"]["local"][sum(counts[:pos])] == s["held"][order[pos]][0]
    # the stamp key at the top position: (4095 * cap + slot) << 1 | 1
    assert ((4095 * facts["cap"] + kept[4095][0]) << 1 | 1) < 1 << 32
    a, b = facts["twice"]
    assert order[a] == order[b] and counts[a] > 0 and counts[b] == 0       # the first occurrence of a keyframe wins
    assert s["held"][order[facts["absent_pos"]]] == [] and order.count(order[facts["absent_pos"]]) == 1
    assert lm.first_occurrence_scan(order, s["held"], s["pt_bad"]) == w["points"]["local"]


@pytest.mark.parametrize("name,n_local", [("f", 32768), ("f1", 32769)])
def test_f_output_capacity(name, n_local):
    s, facts = ms.case(name)
    w = ms.want(name)[0]
    # mcap = 32768: the last output row, and one id that does not fit
    assert len(w["points"]["local"]) == n_local == facts["n_local"] and len(set(w["points"]["local"])) == n_local
    assert w["kf"]["local_kf"] == list(range(64)) and max(len(h) for h in s["held"]) == facts["cap"] == 600
    kept = _kept(name)
    assert all(len(r) >= 512 and {i // LM_NT for i in r} == {0, 1, 2} for r in kept)


def test_g_lines_with_full_rows():
    s, facts = ms.case("g")
    w = ms.want("g")[0]
    assert {len(h) for h in s["lheld"]} == {256} and len(s["frames"][0]["lheld"]) == 256 == facts["klcap"]
    kept = _kept("g", lines=True)
    # klcap = 256: the line rows fill exactly one chunk of k_lm_write; later keyframes still add lines
    assert len(w["lines"]["local"]) > 256 and all(len(r) > 0 for r in kept) and 255 in {r[-1] for r in kept}
    assert lm.first_occurrence_scan(w["kf"]["local_kf"], s["lheld"], s["ln_bad"]) == w["lines"]["local"]


def test_h_the_point_table_of_a_million():
    s, facts = ms.case("h")
    w = ms.want("h")
    for x in w:                                                            # ids 0 and n_pts - 1 are local and held by the frame
        loc = x["points"]["local"]
        assert facts["first"] in loc and facts["last"] in loc
        assert x["points"]["flags"][loc.index(facts["first"])] & 1 == 0 and x["points"]["flags"][loc.index(facts["last"])] & 1 == 0
        assert lm.first_occurrence_scan(x["kf"]["local_kf"], s["held"], s["pt_bad"]) == loc
    a, sh = ms.packed("h")
    e = ls.expected(s, a, sh, 256, 16, w)
    A, SH, E = ms.pad_points(a, sh, e)
    top = ms.MAX_PTS - 1
    assert SH["n_pts"] == 1 << 20 and len(A["pt_flags"]) == 1 << 20 and A["pt_desc"].shape == (1 << 20, 32) and len(A["obs_off"]) == (1 << 20) + 1
    assert (np.diff(A["obs_off"]) >= 0).all() and A["obs_off"][-1] == sh["n_obs_total"]
    assert A["obs_off"][top + 1] - A["obs_off"][top] == a["obs_off"][200] - a["obs_off"][199] and (A["cur_held"][:, 1] == top).all()
    assert (E["local_id"] == top).sum() == 3 and (E["local_id"] == facts["last"]).sum() == 0 and a["pt_xyz"].shape == (200, 3)
    for f in range(3):
        j = int(np.flatnonzero(E["local_id"][f] == top)[0])
        assert E["mp_desc"][f, j].tobytes() == A["pt_desc"][top].tobytes() and E["mp_xyz"][f, j].tobytes() == A["pt_xyz"][top].tobytes()


# ---- i, j: k_cull_kf ---------------------------------------------------------------------------------------------------------------------
def test_i_cull_the_whole_table():
    s, facts = ms.case("i")
    w = ms.want("i")
    rows, order = w[0]
    cand = s["items"][0]
    assert len(s["items"]) == 4096 and sorted(cand) == list(range(4096)) and max(len(h) for h in s["held"]) == facts["cap"] == 8
    # the LDS bitmap s_culled: words 0, 63 and 127 are written first, and the walk of 4096 candidates writes most of the others
    assert order[:3] == facts["early"] == cand[:3] and [k >> 5 for k in order[:3]] == [0, 63, 127]
    assert len({k >> 5 for k in order}) > 100 and len(order) > 500
    # late candidates read the bitmap: the points they share with the early keyframes changed n_redundant and n_gone
    for b in facts["late"]:
        assert cand.index(b) >= 4093 and rows[cand.index(b)] == facts["late_after"] and cm.cull_keyframes(s, [b])[0] == [facts["late_entry"]]
    assert facts["origin"] > 4064 and rows[cand.index(facts["origin"])] == (0, 0, 0, cm.ORIGIN)
    assert facts["held_back"] > 4064 and rows[cand.index(facts["held_back"])] == (8, 8, 0, cm.NOT_ERASE)
    assert sum(1 for r in rows if r[2] > 0) > 20                           # n_gone along the chain
    # one bitmap per item: the late keyframe after its early one, and after another keyframe
    short = [(c, r) for c, (r, _) in zip(s["items"][1:], w[1:]) if len(c) == 2]
    assert len(short) > 4000
    assert all(r[1] == (facts["late_after"] if c[0] in facts["early"] else facts["late_entry"]) for c, r in short if c[0] not in facts["late"])
    assert {c[0] in facts["early"] for c, _ in short} == {True, False} and len({c[0] for c in s["items"]}) > 2000
    for f in (0, 64, 4095):
        assert cm.cull_keyframes_literal(s, s["items"][f])[:2] == w[f]


def test_j_cull_full_keyframes():
    s, facts = ms.case("j")
    w = ms.want("j")
    assert [len(h) for h in s["held"]] == [8192] * 6
    # 10 * n_redundant > 9 * n_mps on either side of nine tenths at n_mps = 8192, and at 8191
    assert w[0][0] == facts["rows"] and w[0][1] == [1, 2, 3]
    assert 10 * 7372 <= 9 * 8192 < 10 * 7373 and 10 * 7371 <= 9 * 8191 < 10 * 7372
    # the slots that decide lie in all eight rounds of the slot loop and in all sixteen waves, so every wave partial sum counts
    for c in range(4):
        plain = facts["not_redundant"][c]
        assert {i // LKF_NT for i in plain} == set(range(8)) and {i % LKF_NT // WAVE for i in plain} == set(range(16))
    # kf_holds falls back to the scan for two slots above 1024 of the culled keyframe 1
    ja, jb = facts["swapped"]
    assert min(ja, jb) > LKF_NT and s["held"][1][ja] == jb and (1, ja) in s["pt_obs"][ja] and s["uright"][1][ja] < 0 <= s["uright"][1][jb]
    assert w[0][0][3][2] == 10 == len(facts["weak"]) and cm.cull_keyframes(s, [3])[0][0][2] == 0   # n_gone only after keyframe 1's cull
    for f, c in enumerate(s["items"]):
        assert cm.cull_keyframes_literal(s, c)[:2] == w[f]
    assert cm.cull_keyframes(s, s["items"][0], wrong="entry")[0] != w[0][0]


# ---- k: k_cull_recent --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [cm.RATIO_FLOAT, cm.RATIO_INT])
def test_k_recent_elements_tiled(form):
    from tests.test_cull_gpu import ELEMENTS, recent_model
    n = ms.MAX_RECENT
    a, want = ms.recent_tiled(n, 3, form)
    assert len(want) == n == 1 << 20 and all(len(v) == n for v in a.values()) and len(ELEMENTS) % LM_NT != 0
    tail = {k: v[n - 700:] for k, v in a.items()}                          # the tiled model is the model of the tiled elements
    assert np.array_equal(recent_model(tail, 3, form), want[n - 700:])
    h, hw = ms.recent_tiled(n, 3, form, host=True)
    assert cm.RECENT_INVALID not in hw and len(hw) == n


def test_the_packed_shapes_are_the_limits():
    """What the GPU suite passes: every limit of the issue's table is reached by some case."""
    sh = {name: ms.packed(name)[1] for name in "abcdefgij"}
    assert sh["a"]["n_tab"] == sh["b"]["n_tab"] == sh["e"]["n_tab"] == sh["i"]["n_tab"] == 4096 and sh["b"]["ccap"] == sh["i"]["ccap"] == 4096
    assert sh["c"]["cap"] == sh["d"]["cap"] == sh["j"]["cap"] == 8192 and sh["g"]["klcap"] == sh["g"]["lcap"] == 256
    assert sh["i"]["n_items"] == 4096 and sh["f"]["cap"] == 600 and sh["a"]["cap"] == 8 and sh["e"]["cap"] == 4
    assert ms.packed("b")[0]["conn"].shape == (4096, 4096) and ms.packed("b")[0]["n_conn"].max() == 4096
    assert ms.packed("i")[0]["cand"].shape == (4096, 4096) and ms.packed("i")[0]["n_cand"][0] == 4096
    a, s2 = ms.packed("d")
    b = ms.absent_ids(a, s2)
    assert (a["cur_held"] == -1).sum() > 100 and (b["cur_held"] == -1).sum() == 0 and (b["held_id"] == -1).sum() == 0
    assert a["cur_held"][0, 8192 - 256 + 2] == -1 and b["cur_held"][0, 8192 - 256 + 2] not in range(s2["n_pts"])

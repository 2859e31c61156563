"""tests/localmap_model.py against hand-worked cases, one per pin of msl_local_keyframes / msl_local_points that msl.h states, and its
properties on random keyframe graphs.  Runs without a GPU."""
import pytest

from tests import localmap_model as lm
from tests import localmap_scenes as ls


def kf_of(scene, frame=0):
    return lm.update_local_map(scene, scene["frames"][frame])["kf"]


def test_votes_count_slots_and_bad_keyframes_and_clear_bad_points():
    s = ls.graph(4, kf_bad=(2,))
    a, b, c = ls.add_point(s, [0, 2]), ls.add_point(s, [1], bad=True), ls.add_point(s, [3])
    s["frames"].append(dict(held=[a, None, b, a, c], lheld=[], prev=[]))
    r = kf_of(s)
    assert r["votes"] == {0: 2, 2: 2, 3: 1}                               # a sits in two slots and votes twice; bad keyframe 2 is counted
    assert r["cleared"] == [2] and r["local_kf"] == [0, 3] and r["ref_kf"] == 0 and r["status"] == 0


def test_empty_counter_keeps_the_old_list():
    s = ls.graph(3)
    b = ls.add_point(s, [1], bad=True)
    s["frames"].append(dict(held=[None, b], lheld=[], prev=[2, 0]))
    r = kf_of(s)
    assert r == dict(votes={}, local_kf=[2, 0], ref_kf=None, cleared=[1], status=lm.NO_VOTES)
    s["held"][2] = [b, None]
    q = ls.add_point(s, [])
    s["held"][0] = [q]
    assert lm.update_local_map(s, s["frames"][0])["points"]["local"] == [q]   # UpdateLocalPoints runs over the old list


def test_first_loop_is_ascending_skips_bad_and_takes_the_lowest_of_equal_maxima():
    s = ls.vote_scene(6, {5: 2, 1: 3, 3: 3, 0: 3}, kf_bad=(0,))
    r = kf_of(s)
    assert r["local_kf"] == [1, 3, 5] and r["ref_kf"] == 1                 # 0 has the same maximum but is bad
    s = ls.vote_scene(3, {0: 1, 2: 4}, kf_bad=(0, 2))
    assert kf_of(s) == dict(votes={0: 1, 2: 4}, local_kf=[], ref_kf=None, cleared=[], status=0)


def test_second_loop_takes_one_neighbour_one_child_and_the_parent():
    # 0: neighbours 1 (in the list), 2 (bad), 3 -> 3; children 4 (bad), 5, 6 -> 5; no parent.  1: nothing new among its ten best, parent 7 (bad) -> 7, stop
    conn = {0: [1, 2, 3, 8], 1: [0, 3, 5, 0, 0, 0, 0, 0, 0, 0, 9], 9: [8]}
    s = ls.vote_scene(10, {0: 1, 1: 1, 9: 1}, conn=conn, parent={4: 0, 5: 0, 6: 0, 1: 7}, kf_bad=(2, 4, 7))
    assert kf_of(s)["local_kf"] == [0, 1, 9, 3, 5, 7]                      # 9 is never walked: the parent's break leaves the walk
    s["parent"][1] = None
    assert kf_of(s)["local_kf"] == [0, 1, 9, 3, 5, 8]                      # the eleventh neighbour of 1 is not looked at; 9 adds 8


def test_second_loop_walks_the_first_loop_s_entries_only():
    s = ls.vote_scene(4, {0: 1}, conn={0: [1], 1: [2], 2: [3]})
    assert kf_of(s)["local_kf"] == [0, 1]


@pytest.mark.parametrize("first,tail", [(78, [100, 103, 101, 104, 128]), (80, [100, 103]), (81, []), (90, [])])
def test_the_stop_above_eighty(first, tail):
    # keyframe 0 adds its neighbour 100 and its child 103 and has no parent; keyframe 1 adds 101, 104 and its parent 128, which ends the walk
    r = kf_of(ls.stop_scene(first))
    assert r["local_kf"] == list(range(first)) + tail                      # 78 ends at 83; 80 stops at the top of the second iteration


def test_composition_flags_and_order():
    s = ls.graph(3)
    p0, p1, p2, p3 = ls.add_point(s, [2, 0]), ls.add_point(s, [0], bad=True), ls.add_point(s, [0, 2], nobs=0), ls.add_point(s, [2])
    s["held"][2].append(p0)                                                # twice in keyframe 2
    s["frames"].append(dict(held=[p0, p1, None], lheld=[0, None], prev=[]))
    s["lheld"][0] = [None, 0, 0]
    r = lm.update_local_map(s, s["frames"][0])
    assert r["kf"]["local_kf"] == [0, 2] and r["kf"]["cleared"] == [1]
    assert r["points"] == dict(local=[p0, p2, p3], flags=[2, 1, 3], cur_flags=[3, 0, 0])   # p0 is held by the frame: no candidate
    assert r["lines"] == dict(local=[0], flags=[2], cur_flags=[3, 0])


@pytest.mark.parametrize("seed", range(6))
def test_properties_on_random_graphs(seed):
    s = ls.random_scene(seed, n_tab=(3, 40, 130)[seed % 3], cap=(5, 30)[seed % 2], n_pts=150, frame_sizes=[0, 5, 30], klcap=4, lcap=4)
    for f, r in zip(s["frames"], ls.model(s)):
        kf = r["kf"]
        live = [k for k in kf["votes"] if not s["kf_bad"][k]]
        assert len(set(kf["local_kf"])) == len(kf["local_kf"])
        if kf["status"] == 0:
            assert kf["local_kf"][:len(live)] == sorted(live)
            assert (kf["ref_kf"] is None) == (not live)
            if live:
                top = max(kf["votes"][k] for k in live)
                assert kf["ref_kf"] == min(k for k in live if kf["votes"][k] == top)
        else:
            assert kf["local_kf"] == f["prev"] and not kf["votes"]
        for name, table, bad in (("points", s["held"], s["pt_bad"]), ("lines", s["lheld"], s["ln_bad"])):
            loc = r[name]["local"]
            assert len(set(loc)) == len(loc) and not any(bad[p] for p in loc)
            assert loc == lm.first_occurrence_scan(kf["local_kf"], table, bad)

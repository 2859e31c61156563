"""tests/kfplanes_model.py against itself: the array form the kernels are compared with equals the literal twin on random plane graphs
carried over 32 consecutive keyframes per seed (bad planes, rows held twice in a frame, outliers, a map-plane table that runs full); the
twin's Map flattened with plane.sort_full / sort_part is the array tables; every inserted key is found by manhattan_model._lookup with the
indices DetectManhattan would read; a second observe of the same keyframe adds nothing; a dot product equal to the threshold is not
vertical.  Runs without a GPU."""
import numpy as np
import pytest

from tests import kfplanes_model as kp
from tests import kfplanes_scenes as ks
from tests import manhattan_model as mh

PCAP, MCAP, FCAP, QCAP, KCAP, N_KF = 8, 32, 3000, 1000, 40, 32


def _state():
    a = dict(frames=np.zeros(1, np.dtype([("enable", "<i4"), ("kf_slot", "<i4"), ("kf_id", "<i4"), ("_pad", "<i4")])),
             plane_coef=np.zeros((1, PCAP, 4), np.float32), plane_npts=np.zeros((1, PCAP), np.int32), n_planes=np.zeros(1, np.int32),
             Tcw=np.zeros((1, 12), np.float32), plane_outlier=np.zeros((1, PCAP, 3), np.uint8), plane_match=np.full((1, PCAP, 3), -1, np.int32),
             mp_w=np.zeros((1, MCAP, 4), np.float32), mp_flags=np.zeros((1, MCAP), np.uint8), mp_first_kf=np.zeros((1, MCAP), np.int32),
             n_map=np.zeros(1, np.int32), kf_Rwc=np.zeros((1, KCAP, 9), np.float32), kf_coef=np.zeros((1, KCAP, PCAP, 4), np.float32),
             kf_npts=np.zeros((1, KCAP, PCAP), np.int32), full_tab=np.zeros((1, FCAP, 7), np.int32), n_full=np.zeros(1, np.int32),
             part_tab=np.zeros((1, QCAP, 5), np.int32), n_part=np.zeros(1, np.int32))
    return a


def _ids(planes):
    return [-1 if p is None else p.mnId for p in planes]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_array_model_equals_the_literal_twin_over_consecutive_keyframes(seed):
    from manhattanslam_amd import plane
    rng = np.random.default_rng(9000 + seed)
    world, a = kp.Map(), _state()
    seen = dict(held_twice=0, bad_held=0, outlier=0, no_room=0, triple=0)
    for t in range(N_KF):
        K = int(rng.integers(0, PCAP + 1))
        coef, npts, Tcw, match, outlier = ks.random_keyframe(rng, len(world.planes), K)
        for p in world.planes:                                              # SetBadFlag between two keyframes
            if rng.random() < 0.04:
                p.bad = True
                a["mp_flags"][0, p.mnId] = 0
        mode, kf_id, slot = (kp.INIT if t == 0 else kp.KEYFRAME), 3 * t + 1, t
        ref = lambda m: None if m < 0 else world.planes[m]
        lf = dict(plane_coef=coef, plane_npts=npts, Tcw=Tcw, planes=[ref(m) for m in match[:, 0]], par=[ref(m) for m in match[:, 1]],
                  ver=[ref(m) for m in match[:, 2]], outlier=outlier)
        a["frames"][0] = (1, slot, kf_id, 0)
        a["plane_coef"][0, :K], a["plane_npts"][0, :K], a["n_planes"][0], a["Tcw"][0] = coef, npts, K, Tcw
        a["plane_match"][0], a["plane_outlier"][0] = -1, 0
        a["plane_match"][0, :K], a["plane_outlier"][0, :K, 0] = match, outlier
        before = a["plane_match"].copy()
        kf, rec = kp.create_keyframe(world, lf, kf_id, slot, mode, MCAP)
        po = kp.keyframe_planes(mode, a)
        assert po["kf_plane_match"][0, :K].T.tolist() == [_ids(kf.planes), _ids(kf.par), _ids(kf.ver)]
        assert np.array_equal(po["plane_new"][0, :K], rec["plane_new"]) and np.array_equal(po["obs_add"][0, :K], rec["obs_add"])
        assert np.array_equal(po["status"][0, :K], rec["status"]) and po["set_not_erase"][0] == rec["set_not_erase"]
        assert po["n_new"][0] == rec["plane_new"].sum() and a["n_map"][0] == len(world.planes)
        assert np.array_equal(po["merge_into"][0, :K], np.where(rec["plane_new"] == 1, _ids(kf.planes), -1))
        M = len(world.planes)
        assert a["mp_w"][0, :M].tobytes() == np.array([p.world for p in world.planes], np.float32).reshape(M, 4).tobytes()
        assert a["mp_flags"][0, :M].tolist() == [0 if p.bad else 1 for p in world.planes]
        assert a["mp_first_kf"][0, :M].tolist() == [p.mnFirstKFid for p in world.planes]
        assert a["kf_Rwc"][0, slot].tobytes() == kf.Rwc.tobytes() and po["Twc"][0].tobytes() == kf.Twc.tobytes()
        assert a["kf_coef"][0, slot, :K].tobytes() == kf.coef.tobytes() and not a["kf_coef"][0, slot, K:].any()
        assert a["kf_npts"][0, slot, :K].tolist() == kf.npts.tolist() and not a["kf_npts"][0, slot, K:].any()
        if mode == kp.INIT:
            assert a["plane_match"][0, :K, 0].tolist() == _ids(lf["planes"])
        else:
            assert a["plane_match"].tobytes() == before.tobytes()            # the frame keeps its NULLs (mLastFrame does not hold the new plane)
        # ProcessNewKeyFrame
        keys = (set(world.full), set(world.part))
        recent = kp.process_new_keyframe(world, kf, ks.TH)
        b = dict(a, kf_plane_match=po["kf_plane_match"])
        oo = kp.manhattan_observe(ks.TH, b, KCAP)
        full, part = world.tables()
        nf, nq = int(a["n_full"][0]), int(a["n_part"][0])
        assert a["full_tab"][0, :nf].tobytes() == plane.sort_full(full).tobytes() and a["part_tab"][0, :nq].tobytes() == plane.sort_part(part).tobytes()
        assert np.array_equal(oo["recent_plane"][0, :K], recent) and oo["status"][0] == 0
        assert oo["added_full"][0] == len(world.full) - len(keys[0]) and oo["added_part"][0] == len(world.part) - len(keys[1])
        assert oo["set_not_erase"][0] == int(kf.not_erase) == int(oo["added_full"][0] + oo["added_part"][0] > 0)
        for w, tab, n, added, old in ((3, a["full_tab"], nf, world.full, keys[0]), (2, a["part_tab"], nq, world.part, keys[1])):
            for key in set(added) - old:                                    # what DetectManhattan finds and reads
                e = mh._lookup(tab[0, :n], w, key)
                assert e is not None and e[w] == slot
                for p in added[key][1]:
                    assert mh._index_in_kf(e, w, p.mnId) == p.GetIndexInKeyFrame(kf) == _ids(kf.planes).index(p.mnId)
        # a second ProcessNewKeyFrame of the same keyframe: every key is there
        tabs = (a["full_tab"].copy(), a["part_tab"].copy())
        again = kp.manhattan_observe(ks.TH, b, KCAP)
        assert again["added_full"][0] == again["added_part"][0] == again["set_not_erase"][0] == 0 and (a["n_full"][0], a["n_part"][0]) == (nf, nq)
        assert a["full_tab"].tobytes() == tabs[0].tobytes() and a["part_tab"].tobytes() == tabs[1].tobytes()
        held = [p.mnId for p in kf.planes if p is not None and not p.bad]
        seen["held_twice"] += len(held) != len(set(held))
        seen["bad_held"] += any(p is not None and p.bad for p in kf.planes)
        seen["outlier"] += bool(outlier.any())
        seen["no_room"] += bool((rec["status"] == kp.NO_ROOM).any())
        seen["triple"] += int(oo["added_full"][0]) > 0
    assert all(v > 0 for v in seen.values()), seen


def _two_planes(x):
    a = _state()
    a["frames"][0] = (1, 0, 0, 0)
    a["plane_coef"][0, :2] = [[1, 0, 0, 0], [x, 1, 0, 0]]
    a["n_planes"][0], a["n_map"][0], a["mp_flags"][0, :2] = 2, 2, 1
    a["kf_plane_match"] = np.full((1, PCAP, 3), -1, np.int32)
    a["kf_plane_match"][0, :2, 0] = [0, 1]
    return a


def test_a_dot_product_equal_to_the_threshold_is_not_vertical():
    th = np.float32(ks.TH)
    below = np.nextafter(th, np.float32(0))
    assert not kp.vertical(np.array([1, 0, 0], np.float32), np.array([th, 1, 0], np.float32), th)
    assert not kp.vertical(np.array([1, 0, 0], np.float32), np.array([-th, 1, 0], np.float32), th)
    assert kp.vertical(np.array([1, 0, 0], np.float32), np.array([below, 1, 0], np.float32), th)
    assert not kp.vertical(np.array([1, 0, 0], np.float32), np.array([np.nan, 1, 0], np.float32), th)
    for x, added in ((th, 0), (-th, 0), (below, 1), (-below, 1)):
        a = _two_planes(x)
        assert kp.manhattan_observe(th, a, KCAP)["added_part"][0] == added and a["n_part"][0] == added


def test_the_ragged_scenes_hold_the_cases_they_name():
    """tests/kfplanes_scenes.py's batch, through the model: the statuses, the NO_ROOM tables and the untouched frame."""
    from manhattanslam_amd import kfplanes
    caps, a = kfplanes.pack(ks.ragged(), ks.PCAP, ks.MCAP, ks.FCAP, ks.QCAP, ks.KCAP)
    assert caps == (ks.PCAP, ks.MCAP, ks.FCAP, ks.QCAP, ks.KCAP) and a["n_planes"].tolist() == [0, 1, 2, 3, 5, 12, 5, 5, 12]
    b, po, oo = ks.expected(a, kp.KEYFRAME)
    st = [po["status"][f, :n].tolist() for f, n in enumerate(a["n_planes"])]
    assert st[1] == [kp.NEW] and st[2] == [kp.HELD, kp.HELD] and st[4] == [kp.HELD, kp.SKIPPED, kp.NEW, kp.HELD, kp.HELD]
    assert st[7] == [kp.HELD, kp.NEW, kp.HELD, kp.NO_ROOM, kp.NO_ROOM] and st[6] == [kp.SKIPPED] * 5 and st[5] == [kp.HELD] * 12
    assert po["obs_add"][4, :5].tolist() == [[1, 1, 0], [0, 0, 0], [1, 0, 1], [1, 0, 0], [0, 0, 0]] and po["obs_add"][2, :2].tolist() == [[1, 0, 0], [1, 0, 0]]
    assert po["set_not_erase"].tolist() == [0, 1, 0, 0, 1, 0, 0, 1, 0] and po["n_new"].tolist() == [0, 1, 0, 0, 1, 0, 0, 1, 0]
    assert oo["status"].tolist() == [0] * 8 + [kp.FULL_NO_ROOM | kp.PART_NO_ROOM]
    assert oo["added_full"].tolist() == [0, 0, 0, 1, 1, oo["added_full"][5], 0, 1, 0] and oo["added_full"][5] > 20
    assert oo["added_part"][2] == 1 and oo["added_part"][3] == 3 and oo["recent_plane"][4, :5].tolist() == [1, 0, 1, 0, 1]
    for k in ("full_tab", "n_full", "part_tab", "n_part"):
        assert b[k][[0, 6, 8]].tobytes() == a[k][[0, 6, 8]].tobytes(), k
    for k in kfplanes.PLANES_INOUT_KEYS:
        assert b[k][6].tobytes() == a[k][6].tobytes(), k
    # frame 5: the new keys fall before, between and after the old entries, and old entries name rows no frame plane holds
    old = {tuple(e[:3]) for e in a["full_tab"][5, :a["n_full"][5]].tolist()}
    pos = [i for i, e in enumerate(b["full_tab"][5, :b["n_full"][5]].tolist()) if tuple(e[:3]) not in old]
    assert pos[0] > 0 and pos[-1] < b["n_full"][5] - 1 and any(y - x > 1 for x, y in zip(pos, pos[1:])) and len(pos) == oo["added_full"][5]
    assert b["full_tab"][5, :b["n_full"][5]].tolist().count([1, 3, 5, 2, 0, 0, 0]) == 1                  # a key that was there keeps its entry
    # frame 7: new keys before every old entry of non-empty tables (lower bound 0); frame 3: after every old entry
    where = lambda f, tab, n, w: [i for i, e in enumerate(b[tab][f, :b[n][f]].tolist())
                                  if tuple(e[:w]) not in {tuple(x[:w]) for x in a[tab][f, :a[n][f]].tolist()}]
    assert a["n_full"][7] == 2 and where(7, "full_tab", "n_full", 3) == [0] and a["n_part"][7] == 2 and where(7, "part_tab", "n_part", 2) == [0, 2, 3]
    assert b["full_tab"][7, :3].tolist() == [[4, 9, 39, 1, 0, 2, 1], [5, 6, 7, 0, 1, 2, 3], [10, 11, 12, 2, 0, 0, 0]]
    assert a["n_full"][3] == 1 and where(3, "full_tab", "n_full", 3) == [1] and a["n_part"][3] == 2 and where(3, "part_tab", "n_part", 2) == [2, 3, 4]

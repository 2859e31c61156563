"""GPU parity: the batched keyframe search of Tracking::Relocalization (msl_match_keyframe_points[_batch]) vs the sequential CPU model
in tests/reloc_model.py.  Every output must be identical: match_out and nmatches."""
import re

import numpy as np
import pytest

from tests import reloc_model as rm
from tests import reloc_scenes as rs

pytestmark = pytest.mark.gpu

SETTINGS = [(10.0, 100), (3.0, 64)]      # the two calls of Tracking::Relocalization


def _check(p, cur, kf, T, got):
    match, nm = got
    tot = 0
    for f in range(len(cur)):
        wm, wnm = rm.search_keyframe_points(p, cur[f], kf[f], T[f])
        assert nm[f] == wnm, (f, nm[f], wnm)
        assert np.array_equal(match[f], wm), (f, np.flatnonzero(match[f] != wm)[:10])
        tot += wnm
    return tot


@pytest.fixture(scope="module")
def ragged():
    """(params, scene, model outputs) per (th, orb_dist, check_orientation): computed once, shared, never modified."""
    out = {}
    for th, od in SETTINGS:
        for co in (0, 1):
            p = rs.params(th, od, bool(co))
            cur, kf, T = rs.ragged_batch(p)
            out[th, co] = (p, cur, kf, T, [rm.search_keyframe_points(p, cur[f], kf[f], T[f]) for f in range(len(cur))])
    return out


@pytest.mark.parametrize("th,orb_dist", SETTINGS)
@pytest.mark.parametrize("check_orientation", [0, 1])
def test_ragged_batch_matches_model(ragged, th, orb_dist, check_orientation):
    """Eight ragged pairs in one call of the device-indexed form, under both window settings, with and without the rotation check."""
    from manhattanslam_amd import reloc
    p, cur, kf, T, want = ragged[th, check_orientation]
    assert int(p["orb_dist"][0]) == orb_dist
    match, nm = reloc.search_keyframe_points(p, cur, kf, T)
    for f in range(8):
        assert nm[f] == want[f][1], (f, nm[f], want[f][1])
        assert np.array_equal(match[f], want[f][0]), (f, np.flatnonzero(match[f] != want[f][0])[:10])
    assert nm[0] == 0 and nm[2] == 0 and nm[1] == 0                # no keypoints / empty keyframe / the only keypoint held
    assert sum(w[1] for w in want) > 300


def test_a_pair_does_not_depend_on_its_batch_neighbours_and_runs_repeat(ragged):
    from manhattanslam_amd import reloc
    from manhattanslam_amd.match import Matcher
    p, cur, kf, T, want = ragged[10.0, 1]
    m = Matcher()
    a = reloc.search_keyframe_points(p, cur, kf, T, handle=m)
    b = reloc.search_keyframe_points(p, cur, kf, T, handle=m)
    for f in range(8):
        assert np.array_equal(a[0][f], b[0][f]) and a[1][f] == b[1][f]
    for f in (3, 4, 6):                                              # alone, and padded to the batch's capacities
        one = reloc.search_keyframe_points(p, [cur[f]], [kf[f]], T[f:f + 1], handle=m)
        pad = reloc.search_keyframe_points(p, [cur[f]], [kf[f]], T[f:f + 1], handle=m, cap=700, kcap=650)
        assert np.array_equal(one[0][0], want[f][0]) and one[1][0] == want[f][1]
        assert np.array_equal(pad[0][0], want[f][0]) and pad[1][0] == want[f][1]
    order = [6, 4, 3, 0]
    rev = reloc.search_keyframe_points(p, [cur[f] for f in order], [kf[f] for f in order], T[order], handle=m)
    for k, f in enumerate(order):
        assert np.array_equal(rev[0][k], want[f][0]) and rev[1][k] == want[f][1]
    m.close()


def test_host_and_device_memory_give_identical_outputs(ragged):
    """The four combinations of host / device memory on the input and output side; device / device is asynchronous on the handle."""
    import torch
    from manhattanslam_amd import KEYPOINT_DTYPE, reloc
    from manhattanslam_amd._lib import check, lib, ptr
    from manhattanslam_amd.match import Matcher
    p, cur, kf, T, want = ragged[10.0, 1]
    cap, kcap, arrays = reloc.pack_keyframe_points(cur, kf, T)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a.view(np.uint8) if a.dtype == KEYPOINT_DTYPE else a)).cuda()
    d_arrays = [dev(a) for a in arrays]
    torch.cuda.synchronize()
    m = Matcher()
    res = {}
    for mem in (0, 1):
        for out_mem in (0, 1):
            if out_mem:
                mo = torch.full((8, cap), -7, dtype=torch.int32, device="cuda"); nm = torch.full((8,), -7, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
            else:
                mo = np.full((8, cap), -7, np.int32); nm = np.full(8, -7, np.int32)
            ins = d_arrays if mem else arrays
            check(lib.msl_match_keyframe_points(m.h, 8, cap, kcap, ptr(p), *[ptr(a) for a in ins], mem, ptr(mo), ptr(nm), out_mem), "keyframe")
            m.sync()
            res[mem, out_mem] = (mo.cpu().numpy(), nm.cpu().numpy()) if out_mem else (mo, nm)
    # the wrapper for device arrays
    mo = torch.full((8, cap), -7, dtype=torch.int32, device="cuda"); nm = torch.zeros(8, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    reloc.search_keyframe_points_device(m, p, 8, cap, kcap, d_arrays, mo, nm)
    m.sync()
    res["wrapper"] = (mo.cpu().numpy(), nm.cpu().numpy())
    m.close()
    for key, (mo, nm) in res.items():
        for f in range(8):
            n = len(cur[f]["kps"])
            assert np.array_equal(mo[f, :n], want[f][0]) and np.all(mo[f, n:] == -1), (key, f)
            assert nm[f] == want[f][1], (key, f)


def test_full_capacity_pair_with_dense_windows():
    """cap = kcap = 8192, the LDS limit of the assign kernel: windows hold more than the 32 stored candidates and the hand-out needs
    many rounds."""
    from manhattanslam_amd import reloc
    p = rs.params(10.0, 100, True)
    cur, kf, T = rs.random_pair(77, p, n_cur=8192, n_kf=8192, cluster=True)
    tr = {}
    wm, wnm = rm.search_keyframe_points(p, cur, kf, T, tr)
    match, nm = reloc.search_keyframe_points(p, [cur], [kf], T[None])
    assert nm[0] == wnm and np.array_equal(match[0], wm), (nm[0], wnm, np.flatnonzero(match[0] != wm)[:10])
    assert wnm > 2000 and tr["culled"] > 100
    assert sum(1 for a, b in zip(tr["pick"], tr["unconstrained"]) if a >= 0 and b >= 0 and a != b) >= 100      # fall-backs, on the model alone


@pytest.mark.parametrize("nlevels", [1, 16])
def test_pyramids_of_one_and_sixteen_levels(nlevels):
    from manhattanslam_amd import reloc
    p = rs.params(10.0, 100, True, nlevels=nlevels)
    pairs = [rs.random_pair(500 + f, p, n_cur=400 + 37 * f, n_kf=380 + 41 * f, conflict=(f == 1)) for f in range(3)]
    cur = [c for c, _, _ in pairs]; kf = [k for _, k, _ in pairs]; T = np.stack([t for _, _, t in pairs])
    got = reloc.search_keyframe_points(p, cur, kf, T)
    assert _check(p, cur, kf, T, got) > 100


def test_limits_are_refused_without_a_launch():
    """cap / kcap 8193, orb_dist 256 and -1, nlevels 17: MSL_ERR_INVALID with a message, outputs untouched (both forms)."""
    from manhattanslam_amd import MslError, reloc
    from manhattanslam_amd._lib import MSL_MEM_HOST, lib, ptr
    from manhattanslam_amd.match import Matcher
    good = rs.params(10.0, 100, True)
    c, k, t = rs.random_pair(50, good, n_cur=10, n_kf=10)
    m = Matcher()

    def variant(**kw):
        q = good.copy()
        for key, v in kw.items():
            q[key] = v
        return q
    cases = [(8193, 16, good, "cap 8193 outside 1 .. 8192"), (16, 8193, good, "kcap 8193 outside 1 .. 8192"),
             (16, 16, variant(orb_dist=256), "orb_dist 256 outside 0 .. 255"), (16, 16, variant(orb_dist=-1), "orb_dist -1 outside 0 .. 255"),
             (16, 16, variant(nlevels=17), "nlevels 17 outside 1 .. 16")]
    for cap, kcap, p, msg in cases:
        msg = "msl_match_keyframe_points: " + msg
        _, _, arrays = reloc.pack_keyframe_points([c], [k], t[None], cap=cap, kcap=kcap)
        mo = np.full(cap, -7, np.int32); nm = np.full(1, -7, np.int32)
        args = (1, cap, kcap, ptr(p), *[ptr(a) for a in arrays], MSL_MEM_HOST, ptr(mo), ptr(nm), MSL_MEM_HOST)
        assert lib.msl_match_keyframe_points(m.h, *args) == -1 and lib.msl_last_error().decode() == msg     # MSL_ERR_INVALID
        assert lib.msl_match_keyframe_points_batch(0, *args) == -1 and lib.msl_last_error().decode() == msg
        assert np.all(mo == -7) and nm[0] == -7
        with pytest.raises(MslError, match=re.escape(msg) + "$"):
            reloc.search_keyframe_points(p, [c], [k], t[None], cap=cap, kcap=kcap)
    # the limits themselves are accepted, and the handle is still good afterwards
    edge = variant(orb_dist=255)
    got = reloc.search_keyframe_points(edge, [c], [k], t[None], handle=m, cap=8192, kcap=8192)
    _check(edge, [c], [k], t[None], got)
    zero = variant(orb_dist=0)
    got = reloc.search_keyframe_points(zero, [c], [k], t[None], handle=m)
    _check(zero, [c], [k], t[None], got)
    m.close()


# ==== the keyframe database and msl_reloc_candidates ============================================================================================
def _fill(scene):
    """(vocabulary handle, device database, model database, covis, queries) of a database scene, the same adds on both sides."""
    from manhattanslam_amd.bow import Vocabulary
    from manhattanslam_amd.reloc import KeyFrameDatabase
    args, V, kfs, covis, queries = rs.database_scene(**scene)
    voc, db, mdb = Vocabulary(*args), KeyFrameDatabase(), rm.Database()
    for w, v in kfs:
        assert db.add(w, v) == mdb.add(w, v)
    return voc, db, mdb, covis, queries


def _same(got, want_list):
    cand, nc, words, score = got
    for f, (wc, ww, ws) in enumerate(want_list):
        assert nc[f] == len(wc) and cand[f].tolist() == wc[:len(cand[f])], (f, cand[f].tolist(), wc)
        if words is not None:
            assert np.array_equal(words[f], ww), f
            assert score[f].tobytes() == ws.tobytes(), (f, np.flatnonzero(score[f] != ws)[:10])


@pytest.mark.parametrize("scene", rs.DATABASE_SCENES, ids=lambda s: "k%dL%d" % (s["k"], s["L"]))
def test_queries_match_the_model_one_call_or_five(scene):
    """Five consecutive frames in one call against the same five in five calls (the state carry), and one frame alone; with erased slots;
    candidates, mnRelocWords and the float scores as bytes."""
    from manhattanslam_amd import reloc
    voc, db, mdb, covis, queries = _fill(scene)
    voc2, db2, mdb2, _, _ = _fill(scene)
    for s in (3, 17, 18):
        db.erase(s); mdb.erase(s); db2.erase(s); mdb2.erase(s)
    assert db.size() == mdb.size() == (scene["n_kf"], scene["n_kf"] - 3)
    want = [mdb.detect(q["bow_word"], q["bow_value"], covis) for q in queries]
    _same(reloc.reloc_candidates(db, voc, queries, covis), want)
    for f, q in enumerate(queries):
        _same(reloc.reloc_candidates(db2, voc2, [q], covis), [want[f]])
    # a second pass over the same frames sees the scores the first pass left
    want2 = [mdb.detect(q["bow_word"], q["bow_value"], covis) for q in queries]
    _same(reloc.reloc_candidates(db, voc, queries, covis, details=False), want2)
    # ccap smaller than the result: the full count, the first ccap slots
    want3 = [mdb.detect(q["bow_word"], q["bow_value"], covis) for q in queries[:2]]
    got = reloc.reloc_candidates(db, voc, queries[:2], covis, ccap=1)
    assert [len(c) for c in got[0]] == [min(1, len(w[0])) for w in want3]
    _same(got, want3)
    for x in (db, db2, voc, voc2):
        x.close()


def test_interleaved_add_erase_query_empty_and_disjoint():
    from manhattanslam_amd import reloc
    from manhattanslam_amd.match import Matcher
    scene = rs.DATABASE_SCENES[1]
    args, V, kfs, covis, queries = rs.database_scene(**scene)
    from manhattanslam_amd.bow import Vocabulary
    from manhattanslam_amd.reloc import KeyFrameDatabase
    voc, db, mdb, m = Vocabulary(*args), KeyFrameDatabase(), rm.Database(), Matcher()
    # empty database
    got = reloc.reloc_candidates(db, voc, queries[:2], [], handle=m)
    assert got[1].tolist() == [0, 0] and all(len(c) == 0 for c in got[0])
    rng = np.random.default_rng(3)
    live = []
    for step, (w, v) in enumerate(kfs):
        s = db.add(w, v, handle=m)
        assert s == mdb.add(w, v)
        live.append(s)
        if step % 7 == 6:
            e = live.pop(int(rng.integers(len(live))))
            db.erase(e); mdb.erase(e)
        if step % 10 == 9:
            q = queries[(step // 10) % len(queries)]
            _same(reloc.reloc_candidates(db, voc, [q], covis, handle=m), [mdb.detect(q["bow_word"], q["bow_value"], covis)])
    assert db.size() == mdb.size()
    # a query sharing no word with any keyframe
    q = dict(bow_word=np.array([10 ** 6], np.int32), bow_value=np.array([1.0]))
    got = reloc.reloc_candidates(db, voc, [q], covis, handle=m)
    mdb.detect(q["bow_word"], q["bow_value"], covis)
    assert got[1][0] == 0 and not got[2].any() and (got[3] == -1).all()
    with pytest.raises(Exception, match="not a live keyframe"):
        db.erase(live[0]); db.erase(live[0])
    mdb.erase(live[0])
    db.clear(); mdb.clear()
    assert db.size() == (0, 0) and db.add(*kfs[0]) == 0 == mdb.add(*kfs[0])
    _same(reloc.reloc_candidates(db, voc, queries[:1], covis, handle=m), [mdb.detect(queries[0]["bow_word"], queries[0]["bow_value"], covis)])
    m.close(); db.close(); voc.close()


def test_8192_slots_growth_and_the_refused_add():
    """8192 one-word keyframes (the CSR storage moves once, from 4096 to 8192 entries), a query over all of them, the 8193rd add refused.
    Several moves: test_storage_moves_several_times_between_queries."""
    from manhattanslam_amd import MslError, reloc
    from manhattanslam_amd.bow import Vocabulary
    from manhattanslam_amd.reloc import KeyFrameDatabase
    from tests import bow_scenes as S
    voc, db, mdb = Vocabulary(*S.full_vocab(5, k=3, L=3)), KeyFrameDatabase(), rm.Database()
    rng = np.random.default_rng(8)
    words = rng.integers(0, 40, 8192)
    vals = rng.integers(1, 9, 8192) / 8.0
    for s in range(8192):
        assert db.add([words[s]], [vals[s]]) == s
        mdb.add([words[s]], [vals[s]])
    with pytest.raises(MslError, match="8192 slots"):
        db.add([1], [1.0])
    assert db.size() == (8192, 8192)
    covis = [[int(x) for x in rng.integers(0, 8192, 10)] for _ in range(8192)]
    qs = [dict(bow_word=np.arange(0, 40, 2 + f, dtype=np.int32), bow_value=np.full(len(range(0, 40, 2 + f)), 1.0 / len(range(0, 40, 2 + f)))) for f in range(2)]
    want = [mdb.detect(q["bow_word"], q["bow_value"], covis) for q in qs]
    assert len(want[0][0]) > 8
    _same(reloc.reloc_candidates(db, voc, qs, covis), want)
    db.close(); voc.close()


def test_storage_moves_several_times_between_queries():
    """48 keyframes of 1000 words: 48 000 entries, so the words / values storage moves four times (4096 -> 8192 -> 16384 -> 32768 -> 65536
    entries); a query after every eighth add reads what the moves copied."""
    from manhattanslam_amd import reloc
    from manhattanslam_amd.bow import Vocabulary
    from manhattanslam_amd.reloc import KeyFrameDatabase
    from tests import bow_scenes as S
    voc, db, mdb = Vocabulary(*S.full_vocab(5, k=3, L=3)), KeyFrameDatabase(), rm.Database()
    rng = np.random.default_rng(9)
    place = [np.sort(rng.choice(6000, 1000, replace=False)).astype(np.int32) for _ in range(6)]
    covis, n_cand = [], 0
    for s in range(48):
        w = place[s % 6].copy()
        swap = rng.random(1000) < 0.2
        w[swap] = rng.integers(6000, 9000, int(swap.sum()))
        w = np.unique(w)
        v = rng.integers(1, 5, len(w)) / (2.0 * len(w))
        assert db.add(w, v) == mdb.add(w, v) == s
        covis.append([int(x) for x in rng.integers(0, s + 1, 4)])
        if s % 8 == 7:
            q = dict(bow_word=place[s % 6], bow_value=np.full(1000, 1e-3))
            want = mdb.detect(q["bow_word"], q["bow_value"], covis)
            _same(reloc.reloc_candidates(db, voc, [q], covis), [want])
            n_cand += len(want[0])
    assert n_cand >= 6 and sum(len(k.words) for k in mdb.kfs) > 32768
    db.close(); voc.close()


def test_refusals_of_the_query():
    """A vocabulary of another scoring is refused by name; NULL optional outputs are accepted (details=False above).  The wrong-device
    refusals are test_a_vocabulary_or_database_on_another_device_is_refused."""
    from manhattanslam_amd import MslError, reloc
    from manhattanslam_amd.bow import Vocabulary
    from manhattanslam_amd.reloc import KeyFrameDatabase
    from tests import bow_scenes as S
    db = KeyFrameDatabase()
    db.add([1, 2], [0.5, 0.5])
    q = [dict(bow_word=np.array([1], np.int32), bow_value=np.array([1.0]))]
    for sc, name in ((1, "L2_NORM"), (5, "DOT_PRODUCT")):
        voc = Vocabulary(*S.full_vocab(5, k=3, L=3, scoring=sc))
        with pytest.raises(MslError, match=name):
            reloc.reloc_candidates(db, voc, q, [[]])
        voc.close()
    db.close()


def test_a_vocabulary_or_database_on_another_device_is_refused():
    """msl_reloc_candidates with a vocabulary, or a database, that lives on another device than the handle, and msl_kfdb_add through a
    handle of another device: MSL_ERR_INVALID, outputs untouched.  These branches compare device numbers, so they can only be reached with
    two devices; on a single-device machine nothing is run."""
    from manhattanslam_amd import device_count
    if device_count() < 2:
        pytest.skip("needs two devices: the refusals compare the device of the vocabulary / database with the handle's")
    from manhattanslam_amd import MslError, reloc
    from manhattanslam_amd._lib import MSL_MEM_HOST, lib, ptr
    from manhattanslam_amd.bow import Vocabulary
    from manhattanslam_amd.match import Matcher
    from manhattanslam_amd.reloc import KeyFrameDatabase
    from tests import bow_scenes as S
    args = S.full_vocab(5, k=3, L=3)
    m0, m1 = Matcher(0), Matcher(1)
    q = [dict(bow_word=np.array([1], np.int32), bow_value=np.array([1.0]))]
    for vdev, ddev in ((1, 0), (0, 1), (1, 1)):
        voc, db = Vocabulary(*args, device=vdev), KeyFrameDatabase(ddev)
        db.add([1, 2], [0.5, 0.5])
        with pytest.raises(MslError, match="must live on the handle's device 0"):
            reloc.reloc_candidates(db, voc, q, [[]], handle=m0)
        voc.close(); db.close()
    db0 = KeyFrameDatabase(0)
    w, v, n, slot = np.array([1], np.int32), np.array([1.0]), np.array([1], np.int32), np.full(1, -7, np.int32)
    assert lib.msl_kfdb_add(db0.h, m1.h, ptr(w), ptr(v), ptr(n), MSL_MEM_HOST, ptr(slot)) == -1 and slot[0] == -7
    assert db0.size() == (0, 0)
    # all on device 1 is accepted
    voc, db = Vocabulary(*args, device=1), KeyFrameDatabase(1)
    assert db.add([1, 2], [0.5, 0.5], handle=m1) == 0
    assert reloc.reloc_candidates(db, voc, q, [[]], handle=m1)[1][0] == 1
    for x in (voc, db, db0, m0, m1):
        x.close()


# ==== Tracking::Relocalization as one device chain ================================================================================================
def test_device_chain_relocalization():
    """Tracking::Relocalization (src/Tracking.cc:1909-2055) on one matcher handle and one stream, device memory throughout: ORB ->
    msl_bow_transform with the BowVector -> msl_kfdb_add of the keyframes -> msl_reloc_candidates -> msl_match_by_bow (0.75) for every
    candidate -> [the scene's true pose, slightly perturbed, and a reprojection inlier mask in place of PnPsolver] -> msl_pose_optimize ->
    cur_held / kf_flags / pt_ref by torch ops -> msl_match_keyframe_points (10, 100) -> msl_pose_optimize -> (3, 64) -> msl_pose_optimize.
    The nGood branch conditions of :1997-2023 are not applied: every stage runs for every candidate.  The handle runs on the torch stream
    the element-wise ops run on, so nothing waits between the stages but msl_kfdb_add (the count) and the host's read of the candidates.
    A second keyframe is added between two queries in flight order (add -> query -> add -> query): the add waits for the first query's
    event, the second query for the first one's scores.  Every stage is compared with its model fed the inputs the device stage read:
    candidates, words, scores (as bytes), matches, flags and return values identical; poses within 1e-6 (no plane edges)."""
    import math
    import torch
    from manhattanslam_amd import KEYPOINT_DTYPE, ORBextractor, bow, frame_params, lib, pose, reloc, synth
    from manhattanslam_amd._lib import check, ptr
    from manhattanslam_amd.bow import Vocabulary
    from manhattanslam_amd.match import Matcher
    from tests import bow_model as M
    from tests import bow_scenes as S
    from tests import match_scenes as ms
    from tests import pose_model as pm
    from tests import pose_scenes as ps
    W, H, K = 640, 480, 4
    B = K + 1                                                            # frame 0: the lost frame; frames 1..K: the keyframes (slots 0..K-1)
    fx = fy = 525.0; cx, cy, Z = 319.5, 239.5, 2.0
    img0 = synth.orb_frame(synth.ORB_SEED + 3)
    shifts = [(1, -2), (3, -4), (-2, 5), (6, 2), (0, 0)]                 # (rows, columns) every view is shifted by: a fronto-parallel wall at depth Z
    imgs = np.stack([np.roll(img0, sh, (0, 1)) for sh in shifts[:4]] + [synth.orb_frame(synth.ORB_SEED + 8)]).astype(np.uint8)
    t_cam = np.array([[dx * Z / fx, dy * Z / fy, 0.0] for dy, dx in shifts], np.float32)      # Pc = Pw + t_cam[f] (Rcw = I)
    depth = np.full((B, H, W), Z, np.float32)
    fp = frame_params(fx, fy, cx, cy, 40.0, W, H)
    sf, inv_sigma2 = ms.orb_tables(8, 1.2)
    ex = ORBextractor(1000, 1.2, 8, 20, 7, max_batch=B)
    cap = ex.capacity
    vargs = S.random_vocab(123, k=10, L=4, scoring=M.L1_NORM, weighting=M.TF_IDF, p_zero=0.02)
    voc, db, mdb, h = Vocabulary(*vargs), reloc.KeyFrameDatabase(), rm.Database(), Matcher()
    stream = torch.cuda.Stream()
    h.set_stream(stream.cuda_stream)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rng = np.random.default_rng(4)
    covis = [[1, 2], [0, 3], [0, 1], [2]]
    with torch.cuda.stream(stream):
        d_img, d_dep = dev(imgs), dev(depth)
        kps = z((B, cap, 28), torch.uint8); desc = z((B, cap, 32), torch.uint8); un = z((B, cap, 2), torch.float32)
        dp = z((B, cap), torch.float32); ur = z((B, cap), torch.float32); cell = z((B, cap), torch.int32); n = z(B, torch.int32)
        word, node, bw, nw = z((B, cap), torch.int32), z((B, cap), torch.int32), z((B, cap), torch.int32), z(B, torch.int32)
        bv = z((B, cap), torch.float64)
        d_covis, d_tcam, d_sf = dev(reloc.pack_covis(covis, K)), dev(t_cam), dev(sf)
        has_mp = dev((rng.random((B, cap)) < 0.9).astype(np.uint8))     # pMP && !pMP->isBad() of every keyframe keypoint
        cand = [torch.full((1, K), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
        ncand = [z(1, torch.int32) for _ in range(2)]
        qwords = [z((1, K), torch.int32) for _ in range(2)]; qscore = [z((1, K), torch.float32) for _ in range(2)]
        stream.synchronize()
        check(lib.msl_orb_extract_frame_batch(ex._h, ptr(d_img), ptr(d_dep), B, W, H, W, W * H, 4 * W, 4 * W * H, 1, ptr(fp), ptr(kps), ptr(desc),
                                              ptr(un), ptr(dp), ptr(ur), ptr(cell), cap, ptr(n), 1), "orb")
        ex.sync()
        # ComputeBoW of every frame, KeyFrameDatabase::add of the keyframes, DetectRelocalizationCandidates twice around the last add
        check(lib.msl_bow_transform(h.h, voc.h, B, cap, 2, ptr(desc), ptr(n), 1, ptr(word), ptr(node), ptr(bw), ptr(bv), ptr(nw), 1), "transform")
        for f in range(1, K):
            assert db.add(bw[f], bv[f], nw[f:f + 1], handle=h) == f - 1
        reloc.reloc_candidates_device(h, db, voc, 1, cap, K, bw[0:1], bv[0:1], nw[0:1], d_covis, cand[0], ncand[0], qwords[0], qscore[0])
        assert db.add(bw[K], bv[K], nw[K:K + 1], handle=h) == K - 1     # waits for the query in flight before it touches the storage
        reloc.reloc_candidates_device(h, db, voc, 1, cap, K, bw[0:1], bv[0:1], nw[0:1], d_covis, cand[1], ncand[1], qwords[1], qscore[1])
        h.sync()                                                        # the host walks vpCandidateKFs (:1917-1953)
        nh, nwh, bwh, bvh = n.cpu().numpy(), nw.cpu().numpy(), bw.cpu().numpy(), bv.cpu().numpy()
        assert nh.min() > 300
        q = (bwh[0, :nwh[0]], bvh[0, :nwh[0]])
        for f in range(1, B):
            mdb.add(bwh[f, :nwh[f]], bvh[f, :nwh[f]])
            if f in (K - 1, K):
                k = f - (K - 1)
                wc, ww, ws = mdb.detect(q[0], q[1], covis)
                got = cand[k].cpu().numpy()[0]
                assert int(ncand[k][0]) == len(wc) and got[:len(wc)].tolist() == wc and np.all(got[len(wc):] == -7), (k, got, wc)
                assert np.array_equal(qwords[k].cpu().numpy()[0, :len(ww)], ww) and qscore[k].cpu().numpy()[0, :len(ws)].tobytes() == ws.tobytes(), k
        slots = wc
        assert len(slots) >= 1 and all(s < 3 for s in slots)              # views of the same wall, never the unrelated keyframe
        P = len(slots)
        kf = torch.tensor([s + 1 for s in slots], device="cuda")          # the frame of every candidate keyframe
        rep = lambda a: a[0:1].expand(P, *a.shape[1:]).contiguous()
        c_kps, c_desc, c_node, c_n, c_un, c_ur, c_cell = (rep(a) for a in (kps, desc, node, n, un, ur, cell))
        k_kps, k_desc, k_node, k_n, k_un, k_dp, k_flags0 = (a[kf].contiguous() for a in (kps, desc, node, n, un, dp, has_mp))
        k_f32, k_i32 = k_kps.view(torch.float32).reshape(P, cap, 7), k_kps.view(torch.int32).reshape(P, cap, 7)
        k_angle, k_oct = k_f32[:, :, 3].contiguous(), k_i32[:, :, 5].long()
        k_flags0 = (k_flags0 & (torch.arange(cap, device="cuda")[None] < k_n[:, None]).to(torch.uint8)).contiguous()
        # the keyframes' map points: their keypoints back-projected at their depth, in the world; mfMaxDistance / mfMinDistance as
        # MapPoint::UpdateNormalAndDepth sets them (src/MapPoint.cc:309-326)
        Pc = torch.stack([(k_un[:, :, 0] - cx) * k_dp / fx, (k_un[:, :, 1] - cy) * k_dp / fy, k_dp], 2)
        k_xyz = (Pc - d_tcam[kf][:, None, :]).contiguous()
        dmax = Pc.norm(dim=2) * d_sf[k_oct]
        k_dist = torch.stack([dmax / float(sf[7]), dmax], 2).contiguous()
        bow_mo, bow_nm = z((P, cap), torch.int32), z(P, torch.int32)
        check(lib.msl_match_by_bow(h.h, P, cap, ptr(bow.bow_match_params(0.75, True)), ptr(k_desc), ptr(k_angle), ptr(k_node), ptr(k_flags0),
                                   ptr(k_n), ptr(c_kps), ptr(c_desc), ptr(c_node), ptr(c_n), 1, ptr(bow_mo), ptr(bow_nm), 1), "bow")
        # in place of PnPsolver::iterate (:1971): Tcw = the true pose moved by 0.3 degrees and a few millimetres, vbInliers = matches
        # that reproject within 3 pixels under the true pose; mvpMapPoints = where(inlier, match, NULL) (:1985-1993)
        T0 = np.tile(ps.tcw12(ps.rot([1, 2, 3], 0.3), t_cam[0] + np.array([0.004, -0.003, 0.005])), (P, 1)).astype(np.float32)
        d_T = [dev(T0)] + [z((P, 12), torch.float32) for _ in range(3)]
        gat = lambda ref: torch.gather(k_xyz, 1, ref.clamp(min=0).long()[:, :, None].expand(P, cap, 3)) + d_tcam[0]
        pc = gat(bow_mo)
        err = torch.hypot(fx * pc[:, :, 0] / pc[:, :, 2] + cx - c_un[:, :, 0], fy * pc[:, :, 1] / pc[:, :, 2] + cy - c_un[:, :, 1])
        ref_pnp = torch.where((bow_mo >= 0) & (err < 3.0), bow_mo, torch.full_like(bow_mo, -1)).contiguous()
        pose_in = [ref_pnp]                                               # mvpMapPoints as every PoseOptimization reads it
        c = ps.params(inv_level_sigma2=inv_sigma2); c.update(fx=fx, fy=fy, cx=cx, cy=cy, bf=40.0)
        prm = pose.pose_params(c)
        lcap = pcap = 1
        out = z((P, cap), torch.uint8); io_rest = [z((P, lcap), torch.uint8), z((P, pcap, 3), torch.uint8)]
        no_lines = [z((P, lcap, 3), torch.float64), z((P, lcap, 6), torch.float64), z((P, lcap), torch.uint8), z(P, torch.int32),
                    z((P, pcap, 4), torch.float32), z((P, pcap, 12), torch.float32), z((P, pcap), torch.uint8), z(P, torch.int32)]
        ng = [z(P, torch.int32) for _ in range(3)]
        out_before, out_after = [], []

        def optimize(k):                                                  # PoseOptimization number k: d_T[k] -> d_T[k + 1]
            out_before.append(out.clone())
            pose.pose_optimization_device(h, prm, P, (cap, cap, lcap, pcap), [c_kps, c_un, c_ur, pose_in[k], c_n, k_xyz] + no_lines + [d_T[k]],
                                          [out] + io_rest, d_T[k + 1], ng[k])
            out_after.append(out.clone())

        def found(ref):                                                   # sFound as a mask over the keyframe's keypoints
            m = z((P, cap + 1), torch.uint8)
            m.scatter_(1, torch.where(ref >= 0, ref, torch.full_like(ref, cap)).long(), 1)
            return m[:, :cap]

        optimize(0)                                                       # :1995
        s_found = found(ref_pnp)                                          # :1990, before the outliers are dropped
        pt_ref = [torch.where(out != 0, torch.full_like(ref_pnp, -1), ref_pnp).contiguous()]       # :2000-2002
        held, flags, add, nadd, kparams = [], [], [], [], []
        for k, (th, od) in enumerate(SETTINGS):
            if k == 1:
                s_found = found(pt_ref[1])                                # :2015-2018
            held.append((pt_ref[k] >= 0).to(torch.uint8).contiguous())   # CurrentFrame.mvpMapPoints[i] != NULL
            flags.append((k_flags0 & (1 - s_found)).contiguous())         # pMP && !isBad() && !sAlreadyFound.count(pMP)
            add.append(torch.full((P, cap), -7, dtype=torch.int32, device="cuda")); nadd.append(z(P, torch.int32))
            kparams.append(reloc.keyframe_match_params(fp, sf, th, od, np.float32(math.log(1.2)), True))
            reloc.search_keyframe_points_device(h, kparams[k], P, cap, cap, [c_kps, c_un, c_cell, c_desc, c_n, held[k], k_xyz, k_dist, k_desc,
                                                                            k_angle, flags[k], k_n, d_T[k + 1]], add[k], nadd[k])   # :2006 / :2019
            pt_ref.append(torch.where(add[k] >= 0, add[k], pt_ref[k]).contiguous())      # the merge: both are keyframe-indexed
            pose_in.append(pt_ref[k + 1])
            optimize(k + 1)                                               # :2010 / :2024
        h.sync()
    # ---- every stage against its model ----
    host = lambda a: a.cpu().numpy()
    kph = host(kps).view(KEYPOINT_DTYPE).reshape(B, cap)
    dh, nodes, unh, urh, cellh = host(desc), host(node), host(un), host(ur), host(cell)
    V = M.build(*vargs)
    for f in range(B):
        wd, nd_, bow_, _ = M.transform(V, dh[f, :nh[f]], 2)
        assert host(word)[f, :nh[f]].tolist() == wd and nodes[f, :nh[f]].tolist() == nd_
        assert bwh[f, :nwh[f]].tolist() == list(bow_) and bvh[f, :nwh[f]].tobytes() == np.array(list(bow_.values())).tobytes()
    n0 = nh[0]
    fl0, xyzh, disth = host(k_flags0), host(k_xyz), host(k_dist)
    refs, reads, Ts = [host(r) for r in pt_ref], [host(r) for r in pose_in], [host(t) for t in d_T]
    for p_, s in enumerate(slots):
        f, nk = s + 1, nh[s + 1]
        pair = {"kf_desc": dh[f, :nk], "kf_angle": kph[f, :nk]["angle"], "kf_node": nodes[f, :nk], "kf_flags": fl0[p_, :nk],
                "cur_angle": kph[0, :n0]["angle"], "cur_desc": dh[0, :n0], "cur_node": nodes[0, :n0]}
        wm, wn = M.search_by_bow(pair, 0.75, True)
        assert host(bow_mo)[p_, :n0].tolist() == wm and int(bow_nm[p_]) == wn
        assert wn > 20 and (reads[0][p_] >= 0).sum() >= 10, (wn, (reads[0][p_] >= 0).sum())
        assert np.array_equal(reads[0][p_, :n0] >= 0, (np.array(wm) >= 0) & (host(err)[p_, :n0] < 3.0))      # the inlier mask
        assert np.array_equal(refs[0][p_, :n0], np.where(host(out_after[0])[p_, :n0] != 0, -1, reads[0][p_, :n0]))
        for k in range(3):                                                # the three PoseOptimizations
            fr = ps.empty(n0, 0, 0, cap)
            fr.update(octave=kph[0, :n0]["octave"].astype(np.int32), un_xy=unh[0, :n0], uright=urh[0, :n0], xyz=xyzh[p_], Tcw=Ts[k][p_],
                      pt_ref=reads[k][p_, :n0], outlier=host(out_before[k])[p_, :n0])
            rows = []
            wng, wT, wout = pm.pose_optimization(fr, c, rows)
            for kind, idx, x2, th in rows:                                # flags are only defined away from the thresholds (pose_scenes.check_margin)
                assert abs(x2 - th) > 1e-4 * th, ("chi2 too close to its threshold", p_, k, kind, idx, x2, th)
            assert int(ng[k][p_]) == wng and np.array_equal(host(out_after[k])[p_, :n0], wout["outlier"]), (p_, k, int(ng[k][p_]), wng)
            assert np.max(np.abs(Ts[k + 1][p_].astype(np.float64) - wT)) <= 1e-6, (p_, k, Ts[k + 1][p_], wT)
        assert int(ng[0][p_]) >= 10
        for k in range(2):                                                # the two keyframe searches
            cur = dict(kps=kph[0, :n0], un_xy=unh[0, :n0], grid_cell=cellh[0, :n0], desc=dh[0, :n0], held=host(held[k])[p_, :n0])
            kfm = dict(xyz=xyzh[p_, :nk], dist=disth[p_, :nk], desc=dh[f, :nk], angle=kph[f, :nk]["angle"], flags=host(flags[k])[p_, :nk])
            wm, wn = rm.search_keyframe_points(kparams[k], cur, kfm, Ts[k + 1][p_].reshape(3, 4))
            got = host(add[k])[p_]
            assert int(nadd[k][p_]) == wn and np.array_equal(got[:n0], wm) and np.all(got[n0:] == -1), (p_, k, int(nadd[k][p_]), wn)
            # the flags and the merge, restated on the host from what the stage before left
            prev = refs[k][p_, :n0]
            assert np.array_equal(cur["held"], (prev >= 0).astype(np.uint8))
            src = reads[0][p_, :n0] if k == 0 else prev                   # sFound: :1990 for the first search, :2015-2018 for the second
            fnd = np.zeros(cap, np.uint8); fnd[src[src >= 0]] = 1
            assert np.array_equal(host(flags[k])[p_], fl0[p_] & (1 - fnd))
            assert np.array_equal(refs[k + 1][p_, :n0], np.where(wm >= 0, wm, prev))
            assert not (set(wm[wm >= 0].tolist()) & set(prev[prev >= 0].tolist()))    # nothing sFound holds is handed out again
        assert int(nadd[0][p_]) >= 30, int(nadd[0][p_])                   # the coarse window really widens the support
        assert np.max(np.abs(Ts[3][p_].reshape(3, 4)[:, 3] - t_cam[0])) < 0.02   # and the chain ends near the true pose
    for x in (h, db, voc, ex):
        x.close()

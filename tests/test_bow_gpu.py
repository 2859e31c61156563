"""msl_bow_transform, msl_match_by_bow and msl_match_lines_by_descriptor on the MI355X against tests/bow_model.py: bit-identical words,
FeatureVector nodes, BowVector values and matches; determinism, batch independence, memory kinds, limits, and the device chain
ORB -> transform -> SearchByBoW -> SearchByDescriptor -> pose optimisation."""
import numpy as np
import pytest

from tests import bow_model as M
from tests import bow_scenes as S

pytestmark = pytest.mark.gpu

MSL_ERR_INVALID = -1


def _vocab(args):
    from manhattanslam_amd.bow import Vocabulary
    return Vocabulary(*args)


def _check_transform(V, frames, got, levelsup):
    for f, fr in enumerate(frames):
        word, node, bow, fv = M.transform(V, fr["desc"], levelsup)
        g = got[f]
        assert g["word"].tolist() == word, (f, levelsup)
        assert g["node"].tolist() == node, (f, levelsup)
        assert g["bow_word"].tolist() == list(bow), (f, levelsup)
        assert g["bow_value"].tobytes() == np.array(list(bow.values()), np.float64).tobytes(), (f, levelsup)


def _frames(args, seed, sizes):
    return [{"desc": S.frame_descs(seed + i, args, n)} for i, n in enumerate(sizes)]


def test_transform_ragged_batches_every_weighting_and_scoring():
    from manhattanslam_amd import bow
    sizes = [0, 1, 300, 97, 64, 5, 700, 33, 256]
    for wt in range(4):
        for sc in range(6):
            args = S.random_vocab(1000 + 6 * wt + sc, k=3 + (wt + sc) % 8, L=3 + sc % 3, scoring=sc, weighting=wt)
            V, voc = M.build(*args), _vocab(args)
            frames = _frames(args, 40 * wt + sc, sizes)
            for levelsup in (0, 2, 4, args[1], args[1] + 1):
                _check_transform(V, frames, bow.transform(voc, frames, levelsup, cap=700), levelsup)
            voc.close()


def test_transform_wide_nodes_stopped_frames_and_empty_vocabulary():
    from manhattanslam_amd import bow
    # k = 20 (32-lane groups), duplicate siblings, many zero weights; frames at cap = 8192 and empty
    args = S.random_vocab(77, k=20, L=3, p_zero=0.3, p_dup=0.3)
    V, voc = M.build(*args), _vocab(args)
    frames = _frames(args, 5, [8192, 0, 1000, 3, 129, 64, 65, 10])
    _check_transform(V, frames, bow.transform(voc, frames, 1, cap=8192), 1)
    voc.close()
    # every word stopped: all -1, empty BowVector
    k, L, sc, wt, parent, leaf, desc, weight = S.random_vocab(78, k=5, L=2)
    args = (k, L, sc, wt, parent, leaf, desc, np.zeros_like(weight))
    voc = _vocab(args)
    got = bow.transform(voc, _frames(args, 6, [50] * 8), 0)
    assert all((g["word"] == -1).all() and (g["node"] == -1).all() and len(g["bow_word"]) == 0 for g in got)
    voc.close()
    # no flagged node: DBoW2's empty()
    args = (k, L, sc, wt, parent, np.zeros_like(leaf), desc, weight)
    voc = _vocab(args)
    got = bow.transform(voc, _frames(args, 7, [20] * 8), 2)
    assert all((g["word"] == -1).all() and len(g["bow_word"]) == 0 for g in got)
    assert voc.info()["n_words"] == 0
    voc.close()


def test_orbvoc_shape_from_arrays_and_from_text(tmp_path):
    from manhattanslam_amd import bow
    args = S.full_vocab(3, scoring=M.L1_NORM, weighting=M.TF_IDF)
    voc = _vocab(args)
    info = voc.info()
    assert (info["k"], info["L"], info["n_nodes"], info["n_words"]) == (10, 6, 1111111, 10 ** 6)
    path = tmp_path / "voc.txt"
    path.write_text(M.write_text(*args))
    vt = bow.Vocabulary.from_text(path)
    assert vt.info() == info
    frames = _frames(args, 9, [1000, 0, 1, 500, 1000, 8, 300, 1000])
    a = bow.transform(voc, frames, 4)
    b = bow.transform(vt, frames, 4)
    for x, y in zip(a, b):
        for key in x:
            assert x[key].tobytes() == y[key].tobytes()
    V = M.build(*args)
    _check_transform(V, frames[:4], a[:4], 4)
    voc.close(); vt.close()


def _pairs():
    specs = [(0, 0), (1, 1), (300, 280), (8192, 8192), (64, 10), (500, 600), (3, 0), (0, 40), (1000, 900)]
    return [S.bow_pair(500 + i, a, b, n_nodes=2 + i % 5) for i, (a, b) in enumerate(specs)]


def _check_bow_match(pairs, got, ratio, orient):
    m, nm = got
    for f, p in enumerate(pairs):
        wm, wn = M.search_by_bow(p, ratio, orient)
        assert m[f].tolist() == wm, f
        assert nm[f] == wn, f


def test_match_by_bow_ragged_batches():
    from manhattanslam_amd import bow
    pairs = _pairs()
    for ratio, orient in ((0.7, True), (0.75, True), (0.8, False)):
        _check_bow_match(pairs, bow.match_by_bow(pairs, ratio, orient, cap=8192), ratio, orient)


def _line_pairs():
    specs = [(0, 5), (1, 1), (5, 0), (30, 2), (256, 256), (40, 64), (100, 65), (7, 200), (64, 64)]
    return [S.line_pair(700 + i, a, b) for i, (a, b) in enumerate(specs)]


def test_match_lines_by_descriptor_ragged_batches():
    from manhattanslam_amd import bow
    pairs = _line_pairs()
    m, nm, lx, lh = bow.match_lines_by_descriptor(pairs, lcap=256, klcap=256, pose_layout=True)
    for f, p in enumerate(pairs):
        wm, wn = M.search_by_descriptor(p)
        assert m[f].tolist() == wm and nm[f] == wn, f
        n = len(p["cur_ldesc"])
        assert lh[f, :n].tolist() == [1 if q >= 0 else 0 for q in wm]
        for t, q in enumerate(wm):
            if q >= 0:
                assert lx[f, t].tobytes() == p["kf_xyz"][q].tobytes()
            else:
                assert not lx[f, t].any()


def test_determinism_and_batch_independence():
    from manhattanslam_amd import bow
    from manhattanslam_amd.match import Matcher
    args = S.random_vocab(91, k=8, L=4)
    voc = _vocab(args)
    frames = _frames(args, 3, [400, 0, 900, 50, 1, 700, 256, 128])
    h = Matcher()
    a, b = bow.transform(voc, frames, 2, handle=h), bow.transform(voc, frames, 2, handle=h)
    alone = bow.transform(voc, frames[5:6], 2, cap=900)
    for x, y in zip(a, b):
        assert all(x[k].tobytes() == y[k].tobytes() for k in x)
    assert all(a[5][k].tobytes() == alone[0][k].tobytes() for k in alone[0])
    pairs = _pairs()
    r1, r2 = bow.match_by_bow(pairs, handle=h), bow.match_by_bow(pairs, handle=h)
    one = bow.match_by_bow(pairs[5:6], cap=8192)
    assert all(np.array_equal(x, y) for x, y in zip(r1[0], r2[0])) and np.array_equal(r1[1], r2[1])
    assert np.array_equal(r1[0][5], one[0][0]) and r1[1][5] == one[1][0]
    lp = _line_pairs()
    l1, l2 = bow.match_lines_by_descriptor(lp, handle=h), bow.match_lines_by_descriptor(lp, handle=h)
    lone = bow.match_lines_by_descriptor(lp[4:5], lcap=300 - 44, klcap=256)
    assert all(np.array_equal(x, y) for x, y in zip(l1[0], l2[0])) and np.array_equal(l1[1], l2[1])
    assert np.array_equal(l1[0][4], lone[0][0])
    h.close(); voc.close()


def test_memory_kinds_on_one_handle():
    import torch
    from manhattanslam_amd import KEYPOINT_DTYPE, bow, lib
    from manhattanslam_amd._lib import check, ptr
    from manhattanslam_amd.match import Matcher
    args = S.random_vocab(55, k=10, L=4, scoring=M.L2_NORM, weighting=M.TF)
    voc = _vocab(args)
    frames = _frames(args, 12, [200, 1500, 0, 30, 700, 90, 1, 4000])
    ref = bow.transform(voc, frames, 2, cap=4000)
    cap, F = 4000, len(frames)
    desc = np.zeros((F, cap, 32), np.uint8); n = np.array([len(f["desc"]) for f in frames], np.int32)
    for f, fr in enumerate(frames):
        desc[f, :n[f]] = fr["desc"]
    h = Matcher()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for mem, out_mem in ((0, 0), (1, 1), (0, 1), (1, 0)):
        src = (dev(desc), dev(n)) if mem else (desc, n)
        outs = [torch.zeros((F, cap), dtype=torch.int32, device="cuda") for _ in range(3)] + [torch.zeros((F, cap), dtype=torch.float64, device="cuda"),
                                                                                             torch.zeros(F, dtype=torch.int32, device="cuda")]
        if not out_mem:
            outs = [np.zeros((F, cap), np.int32) for _ in range(3)] + [np.zeros((F, cap)), np.zeros(F, np.int32)]
        torch.cuda.synchronize()
        check(lib.msl_bow_transform(h.h, voc.h, F, cap, 2, ptr(src[0]), ptr(src[1]), mem, *[ptr(o) for o in outs], out_mem), "transform")
        h.sync()
        w, nd, bw, bv, nw = [o.cpu().numpy() if out_mem else o for o in outs]
        for f in range(F):
            assert np.array_equal(w[f, :n[f]], ref[f]["word"]) and np.array_equal(nd[f, :n[f]], ref[f]["node"])
            assert np.array_equal(bw[f, :nw[f]], ref[f]["bow_word"]) and bv[f, :nw[f]].tobytes() == ref[f]["bow_value"].tobytes()
    # the handle's buffers grow across transform -> match -> pose-sized calls
    pairs = _pairs()
    _check_bow_match(pairs, bow.match_by_bow(pairs, handle=h), 0.7, True)
    cap2, arrays = bow.pack_match_by_bow(pairs[:3], 8192)
    d = [dev(a.view(np.uint8) if a.dtype == KEYPOINT_DTYPE else a) for a in arrays]
    mo = torch.zeros((3, 8192), dtype=torch.int32, device="cuda"); nm = torch.zeros(3, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    check(lib.msl_match_by_bow(h.h, 3, cap2, ptr(bow.bow_match_params()), *[ptr(a) for a in d], 1, ptr(mo), ptr(nm), 1), "match")
    h.sync()
    for f in range(3):
        wm, wn = M.search_by_bow(pairs[f], 0.7, True)
        assert mo[f, :len(wm)].cpu().tolist() == wm and int(nm[f]) == wn
    h.close(); voc.close()


def test_limits_are_refused_before_any_launch():
    from manhattanslam_amd import MslError, bow, device_count, lib
    from manhattanslam_amd._lib import ptr
    from manhattanslam_amd.match import Matcher
    args = S.random_vocab(66, k=4, L=2)
    voc = _vocab(args)
    h = Matcher()
    desc = np.zeros((1, 8193, 32), np.uint8); n = np.array([5], np.int32)
    outs = [np.zeros((1, 8193), np.int32) for _ in range(2)]
    assert lib.msl_bow_transform(h.h, voc.h, 1, 8193, 0, ptr(desc), ptr(n), 0, ptr(outs[0]), ptr(outs[1]), None, None, None, 0) == MSL_ERR_INVALID
    assert lib.msl_last_error().decode() == "msl_bow_transform: cap 8193 outside 1 .. 8192"
    assert lib.msl_bow_transform(h.h, voc.h, 1, 8192, 0, ptr(desc), ptr(n), 0, ptr(outs[0]), ptr(outs[1]), None, None, None, 0) == 0
    p = S.bow_pair(1, 10, 10)
    for cap, rc in ((8192, 0), (8193, MSL_ERR_INVALID)):
        _, arrays = bow.pack_match_by_bow([p], cap)
        mo, nm = np.zeros((1, cap), np.int32), np.zeros(1, np.int32)
        assert lib.msl_match_by_bow(h.h, 1, cap, ptr(bow.bow_match_params()), *[ptr(a) for a in arrays], 0, ptr(mo), ptr(nm), 0) == rc
        assert rc == 0 or lib.msl_last_error().decode() == "msl_match_by_bow: cap 8193 outside 1 .. 8192"
    lp = S.line_pair(2, 10, 10)
    for lcap, klcap, rc, msg in ((256, 256, 0, None), (257, 256, MSL_ERR_INVALID, "lcap 257 outside 1 .. 256"),
                                 (256, 257, MSL_ERR_INVALID, "klcap 257 outside 1 .. 256")):
        _, _, arrays = bow.pack_lines_by_descriptor([lp], lcap, klcap)
        mo, nm = np.zeros((1, lcap), np.int32), np.zeros(1, np.int32)
        assert lib.msl_match_lines_by_descriptor(h.h, 1, lcap, klcap, *[ptr(a) for a in arrays], 0, ptr(mo), ptr(nm), None, None, 0) == rc
        assert rc == 0 or lib.msl_last_error().decode() == "msl_match_lines_by_descriptor: " + msg
    k, L, sc, wt, parent, leaf, d, w = args
    for kk, LL, ok in ((20, 10, True), (21, 10, False), (20, 11, False)):
        if ok:
            bow.Vocabulary(kk, LL, sc, wt, parent, leaf, d, w).close()
        else:
            with pytest.raises(MslError, match="invalid argument"):
                bow.Vocabulary(kk, LL, sc, wt, parent, leaf, d, w)
    if device_count() >= 2:                                              # a vocabulary on another device is refused
        v1 = bow.Vocabulary(*args, device=1)
        assert lib.msl_bow_transform(h.h, v1.h, 1, 8192, 0, ptr(desc), ptr(n), 0, ptr(outs[0]), ptr(outs[1]), None, None, None, 0) == MSL_ERR_INVALID
        v1.close()
    h.close(); voc.close()


def _chain(translation):
    import torch
    from manhattanslam_amd import KEYPOINT_DTYPE, ORBextractor, bow, frame_params, lib, pose, synth
    from manhattanslam_amd._lib import check, ptr
    from manhattanslam_amd.match import Matcher
    from tests import pose_scenes as ps
    W, H, B = 640, 480, 2
    img0 = synth.orb_frame(synth.ORB_SEED + 3)
    imgs = np.stack([img0, np.roll(img0, (3, -4), (0, 1))]).astype(np.uint8)
    depth = np.full((B, H, W), 2.0, np.float32)
    fx = fy = 525.0; cx, cy = 319.5, 239.5
    fp = frame_params(fx, fy, cx, cy, 40.0, W, H)
    ex = ORBextractor(1000, 1.2, 8, 20, 7, max_batch=B)
    cap = ex.capacity
    args = S.random_vocab(123, k=10, L=4, scoring=M.L1_NORM, weighting=M.TF_IDF, p_zero=0.02)
    voc = _vocab(args)
    h = Matcher()
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_img, d_dep = dev(imgs), dev(depth)
    kps = z((B, cap, 28), torch.uint8); desc = z((B, cap, 32), torch.uint8); un = z((B, cap, 2), torch.float32)
    dp = z((B, cap), torch.float32); ur = z((B, cap), torch.float32); cell = z((B, cap), torch.int32); n = z(B, torch.int32)
    word, node, bw, nw = z((B, cap), torch.int32), z((B, cap), torch.int32), z((B, cap), torch.int32), z(B, torch.int32)
    bv = z((B, cap), torch.float64)
    rng = np.random.default_rng(4)
    kf_flags = dev((rng.random(cap) < 0.9).astype(np.uint8)[None])
    lp = S.line_pair(9, 40, 50)
    lcap = klcap = 64
    _, _, larr = bow.pack_lines_by_descriptor([lp], lcap, klcap)
    d_larr = [dev(a) for a in larr]
    mo, nm = z((1, cap), torch.int32), z(1, torch.int32)
    lmo, lnm, lxyz, lhas = z((1, lcap), torch.int32), z(1, torch.int32), z((1, lcap, 6), torch.float64), z((1, lcap), torch.uint8)
    torch.cuda.synchronize()
    # ORB + Frame steps of both images on the device
    check(lib.msl_orb_extract_frame_batch(ex._h, ptr(d_img), ptr(d_dep), B, W, H, W, W * H, 4 * W, 4 * W * H, 1, ptr(fp), ptr(kps), ptr(desc),
                                          ptr(un), ptr(dp), ptr(ur), ptr(cell), cap, ptr(n), 1), "orb")
    ex.sync()
    kf_angle = kps[0:1].view(torch.float32).reshape(1, cap, 7)[:, :, 3].contiguous()
    # 1. transform of the keyframe (frame 0) and the frame (frame 1); 2. SearchByBoW; 3. SearchByDescriptor
    check(lib.msl_bow_transform(h.h, voc.h, B, cap, 2, ptr(desc), ptr(n), 1, ptr(word), ptr(node), ptr(bw), ptr(bv), ptr(nw), 1), "transform")
    check(lib.msl_match_by_bow(h.h, 1, cap, ptr(bow.bow_match_params(0.7, True)), ptr(desc[0:1]), ptr(kf_angle), ptr(node[0:1]), ptr(kf_flags),
                               ptr(n[0:1]), ptr(kps[1:2]), ptr(desc[1:2]), ptr(node[1:2]), ptr(n[1:2]), 1, ptr(mo), ptr(nm), 1), "bow")
    check(lib.msl_match_lines_by_descriptor(h.h, 1, lcap, klcap, *[ptr(a) for a in d_larr], 1, ptr(lmo), ptr(lnm), ptr(lxyz), ptr(lhas), 1),
          "lines")
    # 4. the pose: xyz = the keyframe's back-projected keypoints (its map points), pt_ref = match_out, line_xyz / line_has from the matcher
    h.sync()
    nh = n.cpu().numpy()
    kf_un, kf_d = un[0].cpu().numpy(), dp[0].cpu().numpy()
    xyz = np.zeros((1, cap, 3), np.float32)
    xyz[0, :, 2] = np.where(kf_d > 0, kf_d, 2.0)
    xyz[0, :, 0] = (kf_un[:, 0] - cx) * xyz[0, :, 2] / fx
    xyz[0, :, 1] = (kf_un[:, 1] - cy) * xyz[0, :, 2] / fy
    line_fn = rng.normal(0, 1, (1, lcap, 3))
    line_fn /= np.linalg.norm(line_fn, axis=2, keepdims=True)
    c = ps.params(); c.update(fx=fx, fy=fy, cx=cx, cy=cy, bf=40.0)
    prm = pose.pose_params(c)
    Tcw = np.array([[1, 0, 0, 0.01, 0, 1, 0, -0.02, 0, 0, 1, 0.0]], np.float32)
    Rcw = ps.rot([0, 0, 1], 1.0).astype(np.float32).reshape(1, 9)
    pcap = 1
    host_in = lambda: [kps[1:2].cpu().numpy(), un[1:2].cpu().numpy(), ur[1:2].cpu().numpy(), mo.cpu().numpy(), nh[1:2].copy(), xyz, line_fn,
                       lxyz.cpu().numpy(), lhas.cpu().numpy(), np.array([len(lp["cur_ldesc"])], np.int32), np.zeros((1, pcap, 4), np.float32),
                       np.zeros((1, pcap, 3, 4), np.float32), np.zeros((1, pcap), np.uint8), np.zeros(1, np.int32), Tcw]
    d_in = [kps[1:2], un[1:2], ur[1:2], mo, n[1:2], dev(xyz), dev(line_fn), lxyz, lhas, dev(np.array([len(lp["cur_ldesc"])], np.int32)),
            z((1, pcap, 4), torch.float32), z((1, pcap, 3, 4), torch.float32), z((1, pcap), torch.uint8), z(1, torch.int32), dev(Tcw)]
    d_io = [z((1, cap), torch.uint8), z((1, lcap), torch.uint8), z((1, pcap, 3), torch.uint8)]
    d_T, d_ng = z((1, 12), torch.float32), z(1, torch.int32)
    caps = (cap, cap, lcap, pcap)
    if translation:
        pose.translation_optimization_device(h, prm, 1, caps, d_in, d_io, d_T, d_ng, rcw=dev(Rcw))
    else:
        pose.pose_optimization_device(h, prm, 1, caps, d_in, d_io, d_T, d_ng)
    h.sync()
    # every stage against the model fed the same downloaded inputs
    V = M.build(*args)
    dh, kh = desc.cpu().numpy(), kps.cpu().numpy().view(KEYPOINT_DTYPE).reshape(B, cap)
    assert nh.min() > 300
    for f in range(B):
        wd, nd_, bow_, _ = M.transform(V, dh[f, :nh[f]], 2)
        assert word[f, :nh[f]].cpu().tolist() == wd and node[f, :nh[f]].cpu().tolist() == nd_
        assert bw[f, :nw[f]].cpu().tolist() == list(bow_) and bv[f, :int(nw[f])].cpu().numpy().tobytes() == np.array(list(bow_.values())).tobytes()
    nodes = node.cpu().numpy()
    pair = {"kf_desc": dh[0, :nh[0]], "kf_angle": kh[0, :nh[0]]["angle"], "kf_node": nodes[0, :nh[0]], "kf_flags": kf_flags.cpu().numpy()[0, :nh[0]],
            "cur_angle": kh[1, :nh[1]]["angle"], "cur_desc": dh[1, :nh[1]], "cur_node": nodes[1, :nh[1]]}
    wm, wn = M.search_by_bow(pair, 0.7, True)
    assert mo[0, :nh[1]].cpu().tolist() == wm and int(nm[0]) == wn
    assert wn > 20                                          # the shifted image really matches through the vocabulary
    lm, ln = M.search_by_descriptor(lp)
    assert lmo[0, :len(lm)].cpu().tolist() == lm and int(lnm[0]) == ln
    # the pose equals a host-memory run of the same sequence
    hin = host_in()
    hio = [np.zeros((1, cap), np.uint8), np.zeros((1, lcap), np.uint8), np.zeros((1, pcap, 3), np.uint8)]
    hT, hng = np.zeros((1, 12), np.float32), np.zeros(1, np.int32)
    fn = lib.msl_pose_optimize_translation if translation else lib.msl_pose_optimize
    extra = [ptr(Rcw)] if translation else []
    check(fn(h.h, 1, cap, cap, lcap, pcap, ptr(prm), *[ptr(a) for a in hin], *extra, 0, *[ptr(a) for a in hio], ptr(hT), ptr(hng), 0), "pose host")
    assert int(d_ng[0]) == int(hng[0]) and d_T.cpu().numpy().tobytes() == hT.tobytes()
    for a, b in zip(d_io, hio):
        assert np.array_equal(a.cpu().numpy(), b)
    assert int(hng[0]) > 0
    h.close(); voc.close(); ex.close()


def test_device_chain_track_reference_keyframe():
    _chain(translation=False)


def test_device_chain_translation_estimation():
    _chain(translation=True)

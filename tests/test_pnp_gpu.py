"""msl_pnp_ransac on the device against its sequential model (tests/pnp_model.py) on the fixed scenes of tests/pnp_scenes.py: flags, counts
and status identical (every scene keeps its inlier decisions 2^-19 from the threshold, tests/test_pnp_model.py::test_margins), poses within
the project's pose tolerances (1e-6 on rotation entries, 1e-5 on translation)."""
import numpy as np
import pytest

from tests import pnp_model as pm
from tests import pnp_scenes as ps

pytestmark = pytest.mark.gpu
R_TOL, T_TOL = 1e-6, 1e-5


def _params(p):
    from manhattanslam_amd import pnp
    return pnp.pnp_params(p["fx"], p["fy"], p["cx"], p["cy"], p["level_sigma2"][:p["nlevels"]], p["probability"], p["min_inliers"],
                          p["max_iterations"], p["min_set"], p["epsilon"], p["th2"], p["n_iterations"])


def _run(names, handle=None, **kw):
    from manhattanslam_amd import pnp
    pairs = [ps.scene(n)[0] for n in names]
    return pnp.pnp_ransac(_params(ps.scene(names[0])[1]), pairs, handle=handle, **kw)


def _check(names, res, handle=None):
    Tcw, inl, ref, ni, st = res
    for f, n in enumerate(names):
        m = ps.model(n)
        assert (int(st[f]), int(ni[f])) == (m["status"], m["n_inliers"]), (n, int(st[f]), int(ni[f]), m["status"], m["n_inliers"])
        assert np.array_equal(inl[f], m["inlier"]) and np.array_equal(ref[f], m["pt_ref"]), n
        d = np.abs(Tcw[f].astype(np.float64) - m["Tcw"].astype(np.float64))
        print(n, "status", int(st[f]), "inliers", int(ni[f]), "max |dR|", d[:, :3].max(), "max |dt|", d[:, 3].max())
        assert d[:, :3].max() <= R_TOL and d[:, 3].max() <= T_TOL, (n, d)
        if m["status"] == 0:
            assert np.array_equal(Tcw[f], np.eye(4, dtype=np.float32)[:3]) and not inl[f].any() and np.all(ref[f] == -1)


@pytest.fixture(scope="module")
def matcher():
    from manhattanslam_amd.match import Matcher
    h = Matcher()
    yield h
    h.close()


def test_ragged_batch(matcher):
    """N = 0, 3 (below minInliers), 10 (= minInliers), 11 and 150 with 40 % outliers in one batch."""
    _check(ps.RAGGED, _run(ps.RAGGED, handle=matcher))


def test_per_hypothesis_stage(matcher):
    """Branch and count of every hypothesis identical to the model's, R and t within the tolerances (the aim: the same bits)."""
    from manhattanslam_amd import pnp
    _run(ps.RAGGED, handle=matcher)
    for f, n in enumerate(ps.RAGGED):
        m = ps.model(n)
        R, t, br, cnt = pnp.debug_hypotheses(matcher, f)
        assert len(br) == m["K"], (n, len(br), m["K"])
        if not m["K"]:
            continue
        print(n, "hypotheses", len(br), "bit-identical poses", int(np.sum([R[k].tobytes() == m["R"][k].tobytes() and t[k].tobytes() == m["t"][k].tobytes()
                                                                          for k in range(len(br))])))
        assert np.array_equal(br, m["branch"]) and np.array_equal(cnt, m["count"]), (n, br, m["branch"], cnt, m["count"])
        ok = np.isfinite(m["R"]).all((1, 2)) & np.isfinite(m["t"]).all(1)
        assert np.array_equal(ok, np.isfinite(R).all((1, 2)) & np.isfinite(t).all(1))
        assert np.abs(R[ok] - m["R"][ok]).max() <= R_TOL and np.abs(t[ok] - m["t"][ok]).max() <= T_TOL


def test_full_tracking_settings(matcher):
    """Tracking's (0.99, 10, 300, 4, 0.5, 5.991) and iterate(5): the first successful Refine() is the model's iteration."""
    from manhattanslam_amd import pnp
    names = ("track_a", "track_b")
    res = _run(names, handle=matcher)
    _check(names, res)
    for f, n in enumerate(names):
        m = ps.model(n)
        assert m["status"] == 1 and int(res[4][f]) == 1
        _, _, _, cnt = pnp.debug_hypotheses(matcher, f)
        assert np.array_equal(cnt, m["count"])                          # the same counts -> the same records -> the same first success
        best, first = 0, -1
        for k, c in enumerate(cnt):                                     # the records up to the model's success: its Refine() is the one
            if c >= m["min_inliers"] and c > best:                      # whose inlier set the device returned
                best, first = int(c), k
                if k == m["first_success"]:
                    break
        assert first == m["first_success"]


def test_no_inlier_set(matcher):
    Tcw, inl, ref, ni, st = res = _run(("no_inliers",), handle=matcher)
    _check(("no_inliers",), res)
    assert int(st[0]) == 0 and int(ni[0]) == 0 and np.array_equal(Tcw[0], np.eye(4, dtype=np.float32)[:3]) and not inl[0].any()


def test_batch_independence(matcher):
    """A pair alone and inside a batch: the same bytes; a second call on the same handle: the same bytes again."""
    batch = _run(ps.RAGGED, handle=matcher)
    alone = _run(("ragged150",), handle=matcher, cap=162, kcap=200)
    again = _run(ps.RAGGED, handle=matcher)
    f = ps.RAGGED.index("ragged150")
    for a, b, c in zip(batch, alone, again):
        assert np.asarray(a[f]).tobytes() == np.asarray(b[0]).tobytes()
        assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, c))


def test_host_and_device_memory(matcher):
    import torch
    from manhattanslam_amd import pnp
    pairs = [ps.scene(n)[0] for n in ps.RAGGED]
    prm = _params(ps.scene("ragged150")[1])
    cap, kcap, arrays = pnp.pack_pnp(pairs)
    host = pnp.pnp_ransac(prm, pairs, handle=matcher)
    B = len(pairs)
    dev = [torch.from_numpy(a.view(np.uint8) if a.dtype.names else (a.view(np.int32) if a.dtype == np.uint32 else a)).cuda() for a in arrays]
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    Tcw, inl, ref, ni, st = z((B, 12), torch.float32), z((B, cap), torch.uint8), z((B, cap), torch.int32), z(B, torch.int32), z(B, torch.int32)
    torch.cuda.synchronize()
    pnp.pnp_ransac_device(matcher, prm, B, cap, kcap, dev, Tcw, inl, ref, ni, st)
    matcher.sync()
    assert Tcw.cpu().numpy().tobytes() == host[0].tobytes() and np.array_equal(ni.cpu().numpy(), host[3]) and np.array_equal(st.cpu().numpy(), host[4])
    for f in range(B):
        n = len(pairs[f]["match"])
        assert np.array_equal(inl.cpu().numpy()[f, :n], host[1][f]) and np.array_equal(ref.cpu().numpy()[f, :n], host[2][f])
        assert not inl.cpu().numpy()[f, n:].any() and np.all(ref.cpu().numpy()[f, n:] == -1)


def test_full_capacity(matcher):
    """cap = 8192 with every match valid, kcap = 32768, max_iterations 8: Refine() over thousands of correspondences."""
    res = _run(("full",), handle=matcher)
    assert len(res[1][0]) == 8192 and ps.model("full")["N"] == 8192 and ps.model("full")["status"] == 1
    _check(("full",), res)


def test_refusals(matcher):
    """MSL_ERR_INVALID before any launch, msl_last_error() naming the field."""
    from manhattanslam_amd import lib, pnp
    from manhattanslam_amd._lib import ptr
    sc = ps.scene("eleven")[0]
    cap, kcap, arrays = pnp.pack_pnp([sc])
    out = [np.zeros(12, np.float32), np.zeros(8192, np.uint8), np.zeros(8192, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)]

    def call(cap=cap, kcap=kcap, **kw):
        p = _params(dict(ps.scene("eleven")[1], **{k: v for k, v in kw.items() if k != "nlevels"}))
        if "nlevels" in kw:
            p["nlevels"] = kw["nlevels"]
        rc = lib.msl_pnp_ransac(matcher.h, 1, cap, kcap, ptr(p), *[ptr(a) for a in arrays], 0, *[ptr(a) for a in out], 0)
        return rc, lib.msl_last_error().decode()

    for kw, field in ((dict(min_set=3), "min_set"), (dict(min_set=5), "min_set"), (dict(cap=8193), "cap"), (dict(kcap=32769), "kcap"),
                      (dict(max_iterations=1025), "max_iterations"), (dict(n_iterations=1025), "n_iterations"), (dict(max_iterations=0), "max_iterations"),
                      (dict(nlevels=0), "nlevels"), (dict(nlevels=17), "nlevels")):
        rc, msg = call(**kw)
        assert rc == -1 and field in msg, (kw, rc, msg)
    assert call()[0] == 0 and out[4][0] == ps.model("eleven")["status"]


def test_chain_bow_pnp_pose():
    """msl_match_by_bow -> msl_pnp_ransac -> msl_pose_optimize on one matcher handle and one torch stream, device tensors throughout: the
    matches of every (lost frame, keyframe) pair go into the PnP call as they are, its pose and pt_ref_out into PoseOptimization with no host
    copy and no element-wise step in between (Tracking.cc:1955-1995).  Views of one image shifted by whole pixels; the keyframes' map points
    are their keypoints back-projected, in the lost frame's camera, at a depth that varies over the image (EPnP needs non-coplanar points).
    Every stage is compared with its model fed the inputs the device stage read."""
    import torch
    from manhattanslam_amd import KEYPOINT_DTYPE, ORBextractor, bow, frame_params, lib, pnp, pose, synth
    from manhattanslam_amd._lib import check, ptr
    from manhattanslam_amd.bow import Vocabulary
    from manhattanslam_amd.match import Matcher
    from tests import bow_model as M
    from tests import bow_scenes as S
    from tests import match_scenes as ms
    from tests import pose_model as pom
    from tests import pose_scenes as pos
    W, H = 640, 480
    fx = fy = 525.0; cx, cy = 319.5, 239.5
    img0 = synth.orb_frame(synth.ORB_SEED + 3)
    shifts = [(1, -2), (3, -4), (-2, 5)]                                  # (rows, columns): frame 0 is the lost frame, 1 and 2 the keyframes
    B, P = len(shifts), len(shifts) - 1
    imgs = np.stack([np.roll(img0, sh, (0, 1)) for sh in shifts]).astype(np.uint8)
    depth = np.full((B, H, W), 2.0, np.float32)
    fp = frame_params(fx, fy, cx, cy, 40.0, W, H)
    sf, inv_sigma2 = ms.orb_tables(8, 1.2)
    ex = ORBextractor(1000, 1.2, 8, 20, 7, max_batch=B)
    cap = ex.capacity
    vargs = S.random_vocab(123, k=10, L=4, scoring=M.L1_NORM, weighting=M.TF_IDF, p_zero=0.02)
    voc, h = Vocabulary(*vargs), Matcher()
    stream = torch.cuda.Stream()
    h.set_stream(stream.cuda_stream)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t0 = np.array([0.1, -0.05, 0.2], np.float32)                          # the lost frame's true pose: Pc = Pw + t0
    sigma2 = (np.asarray(sf, np.float32)[:8] ** 2).astype(np.float32)
    pprm = pnp.pnp_params(fx, fy, cx, cy, sigma2, max_iterations=40)
    with torch.cuda.stream(stream):
        d_img, d_dep = dev(imgs), dev(depth)
        kps = z((B, cap, 28), torch.uint8); desc = z((B, cap, 32), torch.uint8); un = z((B, cap, 2), torch.float32)
        dp = z((B, cap), torch.float32); ur = z((B, cap), torch.float32); cell = z((B, cap), torch.int32); n = z(B, torch.int32)
        word, node, bw, nw = z((B, cap), torch.int32), z((B, cap), torch.int32), z((B, cap), torch.int32), z(B, torch.int32)
        bv = z((B, cap), torch.float64)
        d_t0 = dev(t0)
        stream.synchronize()
        check(lib.msl_orb_extract_frame_batch(ex._h, ptr(d_img), ptr(d_dep), B, W, H, W, W * H, 4 * W, 4 * W * H, 1, ptr(fp), ptr(kps), ptr(desc),
                                              ptr(un), ptr(dp), ptr(ur), ptr(cell), cap, ptr(n), 1), "orb")
        ex.sync()
        check(lib.msl_bow_transform(h.h, voc.h, B, cap, 2, ptr(desc), ptr(n), 1, ptr(word), ptr(node), ptr(bw), ptr(bv), ptr(nw), 1), "transform")
        rep = lambda a: a[0:1].expand(P, *a.shape[1:]).contiguous()
        c_kps, c_desc, c_node, c_n, c_un = (rep(a) for a in (kps, desc, node, n, un))
        c_ur = torch.full((P, cap), -1.0, dtype=torch.float32, device="cuda")   # monocular edges: the map points are not at the sensor's depth
        k_kps, k_desc, k_node, k_n, k_un = (a[1:].contiguous() for a in (kps, desc, node, n, un))
        k_angle = k_kps.view(torch.float32).reshape(P, cap, 7)[:, :, 3].contiguous()
        k_flags = (torch.arange(cap, device="cuda")[None] < k_n[:, None]).to(torch.uint8).contiguous()
        rel = dev(np.array([[shifts[0][1] - sh[1], shifts[0][0] - sh[0]] for sh in shifts[1:]], np.float32))   # where the lost frame sees a keyframe pixel
        uc = k_un + rel[:, None, :]
        d = 2.0 + 0.5 * torch.sin(k_un[:, :, 0] / 50.0) + 0.3 * torch.cos(k_un[:, :, 1] / 40.0)
        k_xyz = (torch.stack([(uc[:, :, 0] - cx) * d / fx, (uc[:, :, 1] - cy) * d / fy, d], 2) - d_t0).contiguous()
        bow_mo, bow_nm = z((P, cap), torch.int32), z(P, torch.int32)
        check(lib.msl_match_by_bow(h.h, P, cap, ptr(bow.bow_match_params(0.75, True)), ptr(k_desc), ptr(k_angle), ptr(k_node), ptr(k_flags),
                                   ptr(k_n), ptr(c_kps), ptr(c_desc), ptr(c_node), ptr(c_n), 1, ptr(bow_mo), ptr(bow_nm), 1), "bow")
        seed = dev(np.array([5, 6], np.int32))
        T1, inl, ref = z((P, 12), torch.float32), z((P, cap), torch.uint8), z((P, cap), torch.int32)
        ni, st = z(P, torch.int32), z(P, torch.int32)
        pnp.pnp_ransac_device(h, pprm, P, cap, cap, [c_kps, c_un, bow_mo, c_n, k_xyz, seed], T1, inl, ref, ni, st)
        c = pos.params(inv_level_sigma2=inv_sigma2); c.update(fx=fx, fy=fy, cx=cx, cy=cy, bf=40.0)
        prm = pose.pose_params(c)
        lcap = pcap = 1
        out = z((P, cap), torch.uint8); io_rest = [z((P, lcap), torch.uint8), z((P, pcap, 3), torch.uint8)]
        no_lines = [z((P, lcap, 3), torch.float64), z((P, lcap, 6), torch.float64), z((P, lcap), torch.uint8), z(P, torch.int32),
                    z((P, pcap, 4), torch.float32), z((P, pcap, 12), torch.float32), z((P, pcap), torch.uint8), z(P, torch.int32)]
        T2, ng = z((P, 12), torch.float32), z(P, torch.int32)
        pose.pose_optimization_device(h, prm, P, (cap, cap, lcap, pcap), [c_kps, c_un, c_ur, ref, c_n, k_xyz] + no_lines + [T1], [out] + io_rest, T2, ng)
        h.sync()
    host = lambda a: a.cpu().numpy()
    nh = host(n)
    kph = host(kps).view(KEYPOINT_DTYPE).reshape(B, cap)
    dh, nodes, unh, urh, xyzh = host(desc), host(node), host(un), host(c_ur), host(k_xyz)
    n0 = nh[0]
    mdl = dict(fx=np.float32(fx), fy=np.float32(fy), cx=np.float32(cx), cy=np.float32(cy), nlevels=8, level_sigma2=sigma2, probability=0.99,
               min_inliers=10, max_iterations=40, min_set=4, epsilon=np.float32(0.5), th2=np.float32(5.991), n_iterations=5)
    for p_ in range(P):
        f, nk = p_ + 1, nh[p_ + 1]
        pair = {"kf_desc": dh[f, :nk], "kf_angle": kph[f, :nk]["angle"], "kf_node": nodes[f, :nk], "kf_flags": host(k_flags)[p_, :nk],
                "cur_angle": kph[0, :n0]["angle"], "cur_desc": dh[0, :n0], "cur_node": nodes[0, :n0]}
        wm, wn = M.search_by_bow(pair, 0.75, True)
        got = host(bow_mo)[p_]
        assert got[:n0].tolist() == wm and int(bow_nm[p_]) == wn and wn > 20
        m = pm.pnp_ransac(mdl, kph[0, :n0]["octave"], unh[0, :n0], got[:n0], xyzh[p_], 5 + p_)
        print("pair", p_, "matches", wn, "status", m["status"], "inliers", m["n_inliers"], "margin", m["margin"])
        assert m["margin"] >= 2.0 ** -19, ("an inlier decision too close to its threshold", p_, m["margin"])
        assert (int(st[p_]), int(ni[p_])) == (m["status"], m["n_inliers"]) and m["status"] == 1
        assert np.array_equal(host(inl)[p_, :n0], m["inlier"]) and np.array_equal(host(ref)[p_, :n0], m["pt_ref"])
        assert not host(inl)[p_, n0:].any() and np.all(host(ref)[p_, n0:] == -1)
        dT = np.abs(host(T1)[p_].reshape(3, 4).astype(np.float64) - m["Tcw"])
        assert dT[:, :3].max() <= R_TOL and dT[:, 3].max() <= T_TOL, dT
        assert np.abs(host(T1)[p_].reshape(3, 4)[:, 3] - t0).max() < 0.02
        fr = pos.empty(n0, 0, 0, cap)
        fr.update(octave=kph[0, :n0]["octave"].astype(np.int32), un_xy=unh[0, :n0], uright=urh[0, :n0], xyz=xyzh[p_], Tcw=host(T1)[p_],
                  pt_ref=host(ref)[p_, :n0], outlier=np.zeros(n0, np.uint8))
        rows = []
        wng, wT, wout = pom.pose_optimization(fr, c, rows)
        for kind, idx, x2, th in rows:
            assert abs(x2 - th) > 1e-4 * th, ("chi2 too close to its threshold", p_, kind, idx, x2, th)
        assert int(ng[p_]) == wng and np.array_equal(host(out)[p_, :n0], wout["outlier"])
        assert np.max(np.abs(host(T2)[p_].astype(np.float64) - wT)) <= 1e-6
        assert wng >= 10
    for x in (h, voc, ex):
        x.close()

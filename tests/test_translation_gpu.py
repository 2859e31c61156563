"""GPU parity: batched translation-only optimisation (msl_pose_optimize_translation[_batch], Optimizer::TranslationOptimization) vs the
sequential CPU model in tests/translation_model.py.  n_good and every outlier byte must be identical (the parallel / vertical plane bytes
untouched); Tcw_out within 1e-6 on frames without plane edges and 1e-5 with them, the tolerances of tests/test_pose_gpu.py for the same
reason.  The scene helper asserts that every final chi2 of the model lies more than 1e-4 (relative) away from its threshold.  Last, the
device chain of Tracking::TranslationWithMotionModel on one handle."""
import numpy as np
import pytest

from tests import pose_scenes as ps
from tests import translation_model as tm
from tests import translation_scenes as ts

pytestmark = pytest.mark.gpu


def _check(c, frames, rcw, got):
    for f, fr in enumerate(frames):
        wn, wT, wout = tm.translation_optimization(fr, c, None if rcw is None else rcw[f])
        n, T, out = got[f]
        assert n == wn, (f, n, wn)
        for k, v in wout.items():
            assert np.array_equal(out[k], v), (f, k, np.flatnonzero(out[k] != v)[:10])
        tol = 1e-5 if np.any(fr["plane_has"]) and wn != 0 else 1e-6
        assert np.max(np.abs(T.astype(np.float64) - wT)) <= tol, (f, T, wT)


def _ragged(c):
    specs = [dict(seed=701, n_pts=0, n_lines=6, n_planes=2),                       # no points
             dict(seed=702, n_pts=2, n_lines=4, n_planes=2, null_frac=0.0),        # fewer than 3 correspondences (lines and planes do not count)
             dict(seed=703, n_pts=0, n_lines=25, n_planes=0),                      # only lines
             dict(seed=704, n_pts=0, n_lines=0, n_planes=5),                       # only planes
             dict(seed=705, n_pts=8192, n_lines=12, n_planes=3),                   # the top end of cap
             dict(seed=706, n_pts=1000, n_lines=30, n_planes=0, outliers=0.3, line_outliers=0.3),   # 30 % outliers
             dict(seed=707, n_pts=5, n_lines=1, n_planes=0, null_frac=0.0),        # 7 edges: stops after the first round
             dict(seed=708, n_pts=600, n_lines=0, n_planes=0, stereo=0.0),         # mono only
             dict(seed=709, n_pts=1000, n_lines=40, n_planes=6)]                   # every kind
    out = [ts.scene(c=c, **s) for s in specs]
    return [o[0] for o in out], np.stack([o[1] for o in out])


def test_ragged_batch_matches_model():
    from manhattanslam_amd import pose
    c = ps.params()
    frames, rcw = _ragged(c)
    got = pose.translation_optimization_batch(pose.pose_params(c), frames, rcw)
    _check(c, frames, rcw, got)
    for f in (0, 1, 2, 3):                                                         # < 3 points: 0, the pose as given apart from Rcw
        assert got[f][0] == 0 and got[f][1].tobytes() == tm.effective_tcw(frames[f]["Tcw"], rcw[f]).tobytes()
        assert np.array_equal(got[f][2]["plane_outlier"], frames[f]["plane_outlier"])
    assert got[5][0] < 800 and got[5][2]["outlier"][frames[5]["pt_ref"] >= 0].sum() > 200   # the gross outliers are flagged
    for f in (4, 5, 8):                                                            # the rotation stays Rcw up to the quaternion round trip
        assert np.max(np.abs(got[f][1].reshape(3, 4)[:, :3] - rcw[f].reshape(3, 3))) <= 2e-7


def test_deterministic_and_independent_of_the_batch():
    from manhattanslam_amd import pose
    from manhattanslam_amd.match import Matcher
    c = ps.params()
    sc = [ts.scene(720 + f, n_pts=400 + 100 * f, n_lines=10, n_planes=3, c=c) for f in range(5)]
    frames, rcw = [s[0] for s in sc], np.stack([s[1] for s in sc])
    p = pose.pose_params(c)
    caps = (1000, 1000, 16, 8)
    a = pose.translation_optimization_batch(p, frames, rcw, caps=caps)
    m = Matcher()
    b = pose.translation_optimization_batch(p, frames, rcw, handle=m, caps=caps)
    alone = pose.translation_optimization_batch(p, [frames[3]], rcw[3:4], handle=m, caps=caps)[0]
    m.close()
    for x, y in zip(a, b):
        assert x[0] == y[0] and x[1].tobytes() == y[1].tobytes() and all(np.array_equal(x[2][k], y[2][k]) for k in x[2])
    assert alone[0] == a[3][0] and alone[1].tobytes() == a[3][1].tobytes()
    assert all(np.array_equal(alone[2][k], a[3][2][k]) for k in alone[2])
    _check(c, frames, rcw, a)


def test_rcw_null_uses_tcw_as_given():
    """Rcw = NULL with Rcw already in Tcw gives the bytes of Rcw given; Rcw = NULL on the original Tcw optimises from its own rotation."""
    from manhattanslam_amd import pose
    c = ps.params()
    sc = [ts.scene(740 + f, n_pts=500, n_lines=8, n_planes=2, c=c) for f in range(3)]
    frames, rcw = [s[0] for s in sc], np.stack([s[1] for s in sc])
    p = pose.pose_params(c)
    given = pose.translation_optimization_batch(p, frames, rcw)
    merged = [dict(fr, Tcw=tm.effective_tcw(fr["Tcw"], r)) for fr, r in zip(frames, rcw)]
    null = pose.translation_optimization_batch(p, merged, None)
    for x, y in zip(given, null):
        assert x[0] == y[0] and x[1].tobytes() == y[1].tobytes() and all(np.array_equal(x[2][k], y[2][k]) for k in x[2])
    own = pose.translation_optimization_batch(p, frames, None)                     # Tcw's own rotation (about 2 degrees off)
    for fr in frames:
        ts.check_margin(fr, c, None)
    _check(c, frames, None, own)
    for f, fr in enumerate(frames):
        assert np.max(np.abs(own[f][1].reshape(3, 4)[:, :3] - fr["Tcw"].reshape(3, 4)[:, :3])) <= 2e-7


@pytest.mark.parametrize("what", ["cap", "xcap", "lcap", "pcap", "nlevels"])
def test_limits_are_refused_without_a_launch(what):
    from manhattanslam_amd import MslError, pose
    c = ps.params()
    fr, rcw, _, _ = ts.scene(750, n_pts=20, n_lines=2, n_planes=1, c=c)
    caps = dict(cap=20, xcap=20, lcap=2, pcap=1)
    big = dict(cap=8193, xcap=32769, lcap=257, pcap=65)
    p = pose.pose_params(c)
    if what == "nlevels":
        p["nlevels"] = 17
    else:
        caps[what] = big[what]
    with pytest.raises(MslError, match=r"\(-1\)"):
        pose.translation_optimization_batch(p, [fr], rcw[None], caps=(caps["cap"], caps["xcap"], caps["lcap"], caps["pcap"]))
    assert pose.translation_optimization_batch(pose.pose_params(c), [fr], rcw[None])[0][0] > 0   # the device is still usable


def test_device_chain_of_translation_with_motion_model(oracle):
    """TranslationWithMotionModel (src/Tracking.cc:946-1050) on one handle, device memory throughout: msl_match_by_projection (th 15) ->
    msl_match_lines_by_projection (th 15, line_xyz / line_has in the pose layout) -> msl_pose_optimize_translation with Rcw, points through
    pt_ref = the point match.  The point matches equal the CPU oracle's, the line matches tests/line_match_model.py's, and the optimiser's
    outputs tests/translation_model.py's fed the same arrays."""
    import torch
    from manhattanslam_amd import KEYLINE_DTYPE, KEYPOINT_DTYPE, MATCH_PARAMS_DTYPE, match, pose
    from manhattanslam_amd.match import Matcher
    from tests import line_match_model as lmm
    from tests import line_match_scenes as lsc
    from tests import local_match_scenes as ls
    from tests import match_scenes as ms
    from tests import oracle_lib
    from tests.test_line_match_gpu import _line_fn
    p = ls.params(3.0)
    pll = lsc.params(15.0)
    pbp = ms.params(None, 15.0, False, dtype=MATCH_PARAMS_DTYPE)
    c = ps.params(); c.update(fx=float(p["fx"][0]), fy=float(p["fy"][0]), cx=float(p["cx"][0]), cy=float(p["cy"][0]), bf=float(p["bf"][0]))
    B = 3
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a.view(np.uint8) if a.dtype in (KEYPOINT_DTYPE, KEYLINE_DTYPE) else a)).cuda()
    # points: the current frame and its local points through the true pose; the last frame = the first 900 of them
    frames = [ls.random_frame(780 + f, p, n_cur=800 + 50 * f, n_local=1200) for f in range(B)]
    cur = [x for x, _, _ in frames]; T = np.stack([t for _, _, t in frames])
    cap, _, arrays = match.pack_local_points(cur, [l for _, l, _ in frames], T)
    kps, un, ur, cell, cdesc, ncur = arrays[:6]
    rng = np.random.default_rng(17)
    lxyz = np.zeros((B, cap, 3), np.float32); ld = np.zeros((B, cap, 32), np.uint8); lfl = np.zeros((B, cap), np.uint8)
    loc = np.zeros((B, cap), np.int32)
    for f, (_, l, _) in enumerate(frames):
        lxyz[f, :900] = l["xyz"][:900]; ld[f, :900] = l["desc"][:900]; lfl[f, :900] = l["flags"][:900] | 1; loc[f, :900] = rng.integers(0, 8, 900)
    # lines: last-frame lines seen from the same poses
    lp = [lsc.frame_pair(790 + f, pll, n_kl=40, n_last=40, noise=0.3, angle_mode="slope", T=T[f]) for f in range(B)]
    lcur = [q[0] for q in lp]; llast = [q[1] for q in lp]
    lcap, llcap, larr = match.pack_lines_last(lcur, llast, T, T)
    m = Matcher()
    zeros = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    out = torch.full((B, cap), -7, dtype=torch.int32, device="cuda"); nmp = zeros(B, torch.int32)
    lmo = torch.full((B, lcap), -7, dtype=torch.int32, device="cuda"); lnm = zeros(B, torch.int32)
    line_xyz = zeros((B, lcap, 6), torch.float64); line_has = zeros((B, lcap), torch.uint8)
    # the optimiser's inputs: mTcw = the true pose with its rotation 1 degree and its translation about 3 cm off; Rcw = the true rotation
    # perturbed by at most 0.5 degrees
    rngp = np.random.default_rng(7)
    Tin = np.zeros((B, 12), np.float32); rcw = np.zeros((B, 9), np.float32)
    for f in range(B):
        R = T[f][:3, :3].astype(np.float64)
        Tin[f] = ps.tcw12(ps.rot(rngp.normal(size=3), 1.0) @ R, T[f][:3, 3] + rngp.normal(size=3) * 0.02)
        rcw[f] = (ps.rot(rngp.normal(size=3), rngp.uniform(0, 0.5)) @ R).astype(np.float32).reshape(9)
    line_fn = np.zeros((B, lcap, 3))
    for f in range(B):
        line_fn[f, :len(lcur[f]["kl"])] = _line_fn(lcur[f]["ends"])
    pcap = 1
    d_kl, d_nkl = dev(larr[0]), dev(larr[2])
    inputs = [dev(kps), dev(un), dev(ur), out, dev(ncur), dev(lxyz), dev(line_fn), line_xyz, line_has, d_nkl, zeros((B, pcap, 4), torch.float32),
              zeros((B, pcap, 12), torch.float32), zeros((B, pcap), torch.uint8), zeros(B, torch.int32), dev(Tin)]
    io = [zeros((B, cap), torch.uint8), zeros((B, lcap), torch.uint8), zeros((B, pcap, 3), torch.uint8)]
    Tout = zeros((B, 12), torch.float32); ng = zeros(B, torch.int32)
    d_rcw = dev(rcw)
    pts = [dev(kps), dev(un), dev(ur), dev(cell), dev(cdesc), dev(ncur), dev(lxyz), dev(ld), dev(lfl), dev(loc), zeros((B, cap), torch.float32),
           dev(np.full(B, 900, np.int32)), dev(T[:, :3, :4].copy()), dev(T[:, :3, :4].copy())]
    lines = [d_kl, dev(larr[1]), d_nkl] + [dev(a) for a in larr[3:]]
    torch.cuda.synchronize()                                         # every fill and upload above ran on torch's stream
    m.search_by_projection_device(pbp, B, cap, pts, out, nmp)
    m.search_lines_by_projection_device(pll, B, lcap, llcap, lines, lmo, lnm, line_xyz, line_has)
    pose.translation_optimization_device(m, pose.pose_params(c), B, (cap, cap, lcap, pcap), inputs, io, Tout, ng, rcw=d_rcw)
    m.sync()
    out_h, nmp_h, lmo_h, lnm_h = out.cpu().numpy(), nmp.cpu().numpy(), lmo.cpu().numpy(), lnm.cpu().numpy()
    lx_h, lh_h, po_h, plo_h = line_xyz.cpu().numpy(), line_has.cpu().numpy(), io[0].cpu().numpy(), io[1].cpu().numpy()
    for f in range(B):
        n, nl = len(cur[f]["kps"]), len(lcur[f]["kl"])
        last = dict(xyz=lxyz[f, :900], desc=ld[f, :900], flags=lfl[f, :900], octave=loc[f, :900], angle=np.zeros(900, np.float32))
        wm, wn = oracle_lib.search_by_projection(pbp, cur[f], last, T[f], T[f])
        assert nmp_h[f] == wn and np.array_equal(out_h[f, :n], wm), f
        wl, wln = lmm.search_lines_by_projection(pll, lcur[f], llast[f], T[f], T[f])
        assert lnm_h[f] == wln and np.array_equal(lmo_h[f, :nl], wl), f
        wx, wh = lmm.pose_layout(wl, llast[f]["xyz"], lcap, np.zeros((lcap, 6)), np.zeros(lcap, np.uint8), clear=True)
        assert lx_h[f].tobytes() == wx.tobytes() and np.array_equal(lh_h[f], wh), f
        fr = ps.empty(n, nl, 0, cap)
        fr.update(octave=cur[f]["kps"]["octave"].astype(np.int32), un_xy=cur[f]["un_xy"], uright=cur[f]["uright"], pt_ref=out_h[f, :n],
                  xyz=lxyz[f], line_fn=line_fn[f, :nl], line_xyz=lx_h[f, :nl], line_has=lh_h[f, :nl], Tcw=Tin[f])
        ts.check_margin(fr, c, rcw[f])
        assert (out_h[f, :n] >= 0).sum() > 150 and lh_h[f, :nl].sum() >= 10          # point and line edges in every frame
        wn_, wT, wout = tm.translation_optimization(fr, c, rcw[f])
        assert int(ng[f]) == wn_ and np.array_equal(po_h[f, :n], wout["outlier"]) and np.array_equal(plo_h[f, :nl], wout["line_outlier"]), f
        assert np.max(np.abs(Tout[f].cpu().numpy().astype(np.float64) - wT)) <= 1e-6, f
        assert wn_ > 100
    m.close()

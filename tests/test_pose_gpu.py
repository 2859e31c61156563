"""GPU parity: batched pose-only optimisation (msl_pose_optimize[_batch], Optimizer::PoseOptimization) vs the sequential CPU model in
tests/pose_model.py.  n_good and every outlier flag must be identical; Tcw_out within 1e-6 on frames without plane edges and 1e-5 with
them (the numeric Jacobian of the plane edges amplifies ulp differences of atan2 / sin / cos and of the summation order).  The scene
helper asserts that every final chi2 of the model lies more than 1e-4 (relative) away from its threshold."""
import math

import numpy as np
import pytest

from tests import local_match_scenes as ls
from tests import pose_model as pm
from tests import pose_scenes as ps

pytestmark = pytest.mark.gpu


def _has_planes(fr):
    return any(np.any(fr[k + "_has"]) for k in ("plane", "par", "ver"))


def _check(c, frames, got):
    for f, fr in enumerate(frames):
        wn, wT, wout = pm.pose_optimization(fr, c)
        n, T, out = got[f]
        assert n == wn, (f, n, wn)
        for k, v in wout.items():
            assert np.array_equal(out[k], v), (f, k, np.flatnonzero(out[k] != v)[:10])
        tol = 1e-5 if _has_planes(fr) else 1e-6
        assert np.max(np.abs(T.astype(np.float64) - wT)) <= tol, (f, T, wT)


def _ragged(c):
    specs = [dict(seed=301, n_pts=0, n_lines=6, n_planes=2),                       # no points
             dict(seed=302, n_pts=2, n_lines=0, n_planes=0, null_frac=0.0),        # fewer than 3 correspondences
             dict(seed=303, n_pts=0, n_lines=25, n_planes=0),                      # only lines
             dict(seed=304, n_pts=0, n_lines=0, n_planes=5),                       # only planes (15 plane edges)
             dict(seed=305, n_pts=8192, n_lines=12, n_planes=3),                   # the top end of cap
             dict(seed=306, n_pts=1000, n_lines=30, n_planes=0, outliers=0.3, line_outliers=0.3),   # 30 % outliers
             dict(seed=307, n_pts=5, n_lines=1, n_planes=0, null_frac=0.0),        # 7 edges: stops after the first round
             dict(seed=308, n_pts=1000, n_lines=40, n_planes=6),
             dict(seed=309, n_pts=600, n_lines=0, n_planes=0, stereo=0.0)]         # mono only
    return [ps.scene(c=c, **s)[0] for s in specs]


def test_ragged_batch_matches_model():
    from manhattanslam_amd import pose
    c = ps.params()
    frames = _ragged(c)
    got = pose.pose_optimization_batch(pose.pose_params(c), frames)
    _check(c, frames, got)
    assert got[1][0] == 0 and np.array_equal(got[1][1], frames[1]["Tcw"])      # < 3 correspondences: 0, pose unchanged
    assert got[5][0] < 800 and got[5][2]["outlier"][frames[5]["pt_ref"] >= 0].sum() > 250   # the gross outliers are flagged


def test_deterministic_and_independent_of_the_batch():
    from manhattanslam_amd import pose
    from manhattanslam_amd.match import Matcher
    c = ps.params()
    frames = [ps.scene(320 + f, n_pts=400 + 100 * f, n_lines=10, n_planes=3, c=c)[0] for f in range(5)]
    p = pose.pose_params(c)
    caps = (1000, 1000, 16, 8)
    a = pose.pose_optimization_batch(p, frames, caps=caps)
    m = Matcher()
    b = pose.pose_optimization_batch(p, frames, handle=m, caps=caps)
    alone = pose.pose_optimization_batch(p, [frames[3]], handle=m, caps=caps)[0]
    m.close()
    for x, y in zip(a, b):
        assert x[0] == y[0] and x[1].tobytes() == y[1].tobytes() and all(np.array_equal(x[2][k], y[2][k]) for k in x[2])
    assert alone[0] == a[3][0] and alone[1].tobytes() == a[3][1].tobytes()
    assert all(np.array_equal(alone[2][k], a[3][2][k]) for k in alone[2])
    _check(c, frames, a)


def test_device_form_chained_from_local_map_search():
    """The pipeline shape: msl_match_local_points' device match_out (an index into mp_xyz, or -1 = the keypoint keeps what it held) and
    the points held before the call become (pt_ref, xyz) with a few torch ops on the device, and feed msl_pose_optimize on the same handle
    with device-resident keypoint arrays.  Same result as the model fed the same arrays."""
    import torch
    from manhattanslam_amd import KEYPOINT_DTYPE, LOCAL_TRACK_DTYPE, match, pose
    from manhattanslam_amd.match import Matcher
    p = ls.params(3.0)
    c = ps.params(); c.update(fx=float(p["fx"][0]), fy=float(p["fy"][0]), cx=float(p["cx"][0]), cy=float(p["cy"][0]), bf=float(p["bf"][0]))
    B = 3
    frames = [ls.random_frame(60 + f, p, n_cur=800 + 50 * f, n_local=2000 + 300 * f) for f in range(B)]
    cur = [x for x, _, _ in frames]; local = [l for _, l, _ in frames]; T = np.stack([t for _, _, t in frames])
    cap, mcap, arrays = match.pack_local_points(cur, local, T)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a.view(np.uint8) if a.dtype == KEYPOINT_DTYPE else a)).cuda()
    d = [dev(a) for a in arrays]
    m = Matcher()
    mo = torch.full((B, cap), -7, dtype=torch.int32, device="cuda"); ntm = torch.zeros(B, dtype=torch.int32, device="cuda")
    nm = torch.zeros(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    m.search_local_points_device(p, B, cap, mcap, d, mo, ntm, nm)
    m.sync()
    # points held before the call (cur_flags bit 0): back-projections of their keypoints at 3 m through the true pose
    pre = np.zeros((B, cap, 3), np.float32)
    for f in range(B):
        n = len(cur[f]["kps"])
        xy = cur[f]["un_xy"].astype(np.float64)
        Pc = np.stack([(xy[:, 0] - c["cx"]) / c["fx"] * 3.0, (xy[:, 1] - c["cy"]) / c["fy"] * 3.0, np.full(n, 3.0)], 1)
        R, t = T[f][:3, :3].astype(np.float64), T[f][:3, 3].astype(np.float64)
        pre[f, :n] = ((Pc - t) @ R).astype(np.float32)
    d_pre = dev(pre)
    held = (d[6] & 1).bool()
    idx = torch.arange(cap, device="cuda", dtype=torch.int32).expand(B, cap)
    pt_ref = torch.where(mo >= 0, mo, torch.where(held, idx + mcap, torch.full_like(mo, -1))).contiguous()
    xyz = torch.cat([d[7].view(B, mcap, 3), d_pre], 1).contiguous()                 # mp_xyz, then the pre-held points
    xcap = mcap + cap
    # initial pose: the true one perturbed by about 1 degree and 3 cm
    rng = np.random.default_rng(5)
    Tin = np.zeros((B, 12), np.float32)
    for f in range(B):
        R0 = ps.rot(rng.normal(size=3), 1.0) @ T[f][:3, :3].astype(np.float64)
        Tin[f] = ps.tcw12(R0, T[f][:3, 3] + rng.normal(size=3) * 0.02)
    lcap, pcap = 1, 1
    zero = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    oct_kps = d[0]
    inputs = [oct_kps, d[1], d[2], pt_ref, d[5], xyz, zero((B, lcap, 3), torch.float64), zero((B, lcap, 6), torch.float64),
              zero((B, lcap), torch.uint8), zero(B, torch.int32), zero((B, pcap, 4), torch.float32), zero((B, pcap, 12), torch.float32),
              zero((B, pcap), torch.uint8), zero(B, torch.int32), dev(Tin)]
    io = [zero((B, cap), torch.uint8), zero((B, lcap), torch.uint8), zero((B, pcap, 3), torch.uint8)]
    Tout = zero((B, 12), torch.float32); ng = zero(B, torch.int32)
    pose.pose_optimization_device(m, pose.pose_params(c), B, (cap, xcap, lcap, pcap), inputs, io, Tout, ng)
    m.sync()
    ref_h, xyz_h, out_h = pt_ref.cpu().numpy(), xyz.cpu().numpy(), io[0].cpu().numpy()
    got = []
    model_frames = []
    for f in range(B):
        n = len(cur[f]["kps"])
        fr = ps.empty(n, 0, 0, xcap)
        fr.update(octave=cur[f]["kps"]["octave"].astype(np.int32), un_xy=cur[f]["un_xy"], uright=cur[f]["uright"], pt_ref=ref_h[f, :n],
                  xyz=xyz_h[f], Tcw=Tin[f])
        ps.check_margin(fr, c)
        model_frames.append(fr)
        got.append((int(ng[f]), Tout[f].cpu().numpy(), dict(outlier=out_h[f, :n], line_outlier=np.zeros(0, np.uint8),
                                                           plane_outlier=np.zeros(0, np.uint8), par_outlier=np.zeros(0, np.uint8),
                                                           ver_outlier=np.zeros(0, np.uint8))))
        assert (ref_h[f, :n] >= mcap).sum() > 50 and (ref_h[f, :n] >= 0).sum() > 400
    _check(c, model_frames, got)
    for f in range(B):                                                               # it converged near the true pose
        R = Tout[f].cpu().numpy().reshape(3, 4)[:, :3].astype(np.float64)
        ang = math.degrees(math.acos(min(1.0, (np.trace(R @ T[f][:3, :3].T.astype(np.float64)) - 1) / 2)))
        assert ang < 0.5, ang
    m.close()


def test_one_handle_grows_its_buffers_across_stages(oracle):
    """One Matcher and host-form calls only: last-frame matching, local-map matching and pose optimisation take turns on it, and every call
    is larger (cap / mcap / xcap) than the last call of its kind, so each one grows buffers of the shared handle.  Every result is the
    oracle's or the sequential model's."""
    from manhattanslam_amd import MATCH_PARAMS_DTYPE, match, pose
    from manhattanslam_amd.match import Matcher
    from tests import match_scenes as ms
    from tests import oracle_lib
    from tests.test_local_match_gpu import _check as check_local
    c = ps.params()
    pp, pl, pbp = pose.pose_params(c), ls.params(3.0), ms.params(None, 15, True, dtype=MATCH_PARAMS_DTYPE)
    caps = {"projection": [], "local": [], "pose": []}
    m = Matcher()
    for r, (n_cur, n_local, n_pts) in enumerate(((200, 300, 80), (600, 1500, 400), (1016, 4000, 1500))):
        pairs = [ms.random_pair(400 + 10 * r + j, pbp, n_cur=n_cur - 40 * j, n_last=n_cur - 60 * j) for j in range(2)]
        cur = [q[0] for q in pairs]; last = [q[1] for q in pairs]; Tc = np.stack([q[2] for q in pairs]); Tl = np.stack([q[3] for q in pairs])
        caps["projection"].append(max(max(len(x["kps"]) for x in cur), max(len(x["xyz"]) for x in last)))
        got, nm = m.search_by_projection_batch(pbp, cur, last, Tc, Tl)
        for f in range(2):
            want, n = oracle_lib.search_by_projection(pbp, cur[f], last[f], Tc[f], Tl[f])
            assert nm[f] == n and np.array_equal(got[f], want), (r, f)

        frames = [ls.random_frame(420 + 10 * r + j, pl, n_cur=n_cur - 30 * j, n_local=n_local - 100 * j) for j in range(2)]
        cur = [x for x, _, _ in frames]; local = [l for _, l, _ in frames]; T = np.stack([t for _, _, t in frames])
        caps["local"].append(match.pack_local_points(cur, local, T)[:2])
        assert check_local(pl, cur, local, T, m.search_local_points_batch(pl, cur, local, T)) > 0

        frames = [ps.scene(440 + 10 * r + j, n_pts=n_pts - 20 * j, n_lines=4 * (r + 1), n_planes=r + 1, c=c)[0] for j in range(2)]
        caps["pose"].append(pose.pack(frames)[0])
        _check(c, frames, pose.pose_optimization_batch(pp, frames, handle=m))
    m.close()
    for kind, seq in caps.items():                                                   # the premise: every call grew the handle's buffers
        assert all(np.all(np.greater(b, a)) for a, b in zip(seq, seq[1:])), (kind, seq)


@pytest.mark.parametrize("what", ["cap", "xcap", "lcap", "pcap", "nlevels"])
def test_limits_are_refused_without_a_launch(what):
    from manhattanslam_amd import MslError, pose
    c = ps.params()
    fr = ps.scene(330, n_pts=20, n_lines=2, n_planes=1, c=c)[0]
    caps = dict(cap=20, xcap=20, lcap=2, pcap=1)
    big = dict(cap=8193, xcap=32769, lcap=257, pcap=65)
    p = pose.pose_params(c)
    if what == "nlevels":
        p["nlevels"] = 17
    else:
        caps[what] = big[what]
    with pytest.raises(MslError, match=r"\(-1\)"):
        pose.pose_optimization_batch(p, [fr], caps=(caps["cap"], caps["xcap"], caps["lcap"], caps["pcap"]))
    assert pose.pose_optimization_batch(pose.pose_params(c), [fr])[0][0] > 0       # the device is still usable

"""Synthetic PoseOptimization inputs (fixed seeds) for the model tests and the GPU parity tests: a true camera pose, map points seen by
it (mono and stereo keypoints with octaves), map lines (endpoints + the observed 2-D line function), map planes with the frame's plane
coefficients and the parallel / vertical plane candidates, then an initial pose perturbed from the true one."""
import math

import numpy as np

from tests import pose_model as pm

FX, FY, CX, CY, BF = 517.3, 516.5, 318.6, 255.3, 40.0
NLEVELS, SCALE = 8, 1.2


def params(angleInfo=0.5, disInfo=50.0, parInfo=0.5, verInfo=0.5, planeChi=100.0, planeChiVP=50.0, aTh=0.86, parTh=0.9, nlevels=NLEVELS,
           scale=SCALE, inv_level_sigma2=None):
    """Model constants c (see pose_model.pose_optimization); the msl_pose_params record is manhattanslam_amd.pose.pose_params(c).
    inv_level_sigma2 (mvInvLevelSigma2, nlevels floats): by default 1 / scale^(2 l) rounded from double; pass match_scenes.orb_tables(..)[1]
    for the table msl_orb_scale_tables gives."""
    f = lambda x: float(np.float32(x))
    inv = np.array([1.0 / (scale ** (2 * l)) for l in range(nlevels)], np.float32) if inv_level_sigma2 is None else \
        np.asarray(inv_level_sigma2, np.float32)
    assert 1 <= len(inv) <= 16
    return dict(fx=f(FX), fy=f(FY), cx=f(CX), cy=f(CY), bf=f(BF), inv_level_sigma2=[float(v) for v in inv], angleInfo=angleInfo,
                disInfo=disInfo, parInfo=parInfo, verInfo=verInfo, planeChi=planeChi, planeChiVP=planeChiVP, aTh=aTh, parTh=parTh)


def rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = math.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * K @ K


def tcw12(R, t):
    return np.concatenate([np.hstack([R, np.asarray(t).reshape(3, 1)])]).astype(np.float32).reshape(12)


def empty(n=0, nl=0, m=0, x=0):
    return dict(octave=np.zeros(n, np.int32), un_xy=np.zeros((n, 2), np.float32), uright=np.full(n, -1, np.float32),
                pt_ref=np.full(n, -1, np.int32), xyz=np.zeros((x, 3), np.float32), outlier=np.zeros(n, np.uint8),
                line_fn=np.zeros((nl, 3)), line_xyz=np.zeros((nl, 6)), line_has=np.zeros(nl, np.uint8), line_outlier=np.zeros(nl, np.uint8),
                plane_coef=np.zeros((m, 4), np.float32), plane_w=np.zeros((m, 4), np.float32), par_w=np.zeros((m, 4), np.float32),
                ver_w=np.zeros((m, 4), np.float32), plane_has=np.zeros(m, np.uint8), par_has=np.zeros(m, np.uint8),
                ver_has=np.zeros(m, np.uint8), plane_outlier=np.zeros(m, np.uint8), par_outlier=np.zeros(m, np.uint8),
                ver_outlier=np.zeros(m, np.uint8), Tcw=np.zeros(12, np.float32))


def scene(seed, n_pts=300, n_lines=10, n_planes=3, stereo=0.6, noise=0.5, outliers=0.0, line_outliers=0.0, rot_deg=2.0, trans=0.05,
          null_frac=0.1, par=True, ver=True, margin=1e-4, c=None, nlevels=NLEVELS, scale=SCALE, xcap=None):
    """One frame.  Returns (fr, Rtrue, ttrue).  noise: pixel sigma of the point / line observations (0 = noiseless); outliers: fraction of
    points whose observation is replaced by a random pixel; null_frac: keypoints without a MapPoint; octaves are drawn from [0, nlevels) and
    scale the noise by scale^octave.  xcap: xyz gets xcap rows instead of n_pts, the referenced points scattered over them (slot xcap - 1
    always referenced) with unrelated filler rows in between.  When margin is set, asserts that every edge's final chi2 in the model lies
    more than margin (relative) away from its threshold."""
    c = c or params(nlevels=nlevels, scale=scale)
    rng = np.random.default_rng(seed)
    R = rot(rng.normal(size=3), rng.uniform(0, 40))
    t = rng.normal(size=3)
    fr = empty(n_pts, n_lines, n_planes, n_pts)
    # points in the camera frame, world = R^T (pc - t)
    z = rng.uniform(0.8, 6.0, n_pts)
    u0 = rng.uniform(10, 630, n_pts)
    v0 = rng.uniform(10, 470, n_pts)
    pc = np.stack([(u0 - CX) / FX * z, (v0 - CY) / FY * z, z], 1)
    pw = (pc - t) @ R
    fr["xyz"][:] = pw.astype(np.float32)
    pcf = (fr["xyz"].astype(np.float64) @ R.T) + t
    fr["octave"][:] = rng.integers(0, nlevels, n_pts)
    sig = np.array([scale ** l for l in range(nlevels)])[fr["octave"]]
    u = pcf[:, 0] / pcf[:, 2] * FX + CX + rng.normal(size=n_pts) * noise * sig
    v = pcf[:, 1] / pcf[:, 2] * FY + CY + rng.normal(size=n_pts) * noise * sig
    ur = u - BF / pcf[:, 2] + rng.normal(size=n_pts) * noise * sig
    bad = rng.random(n_pts) < outliers
    u[bad] = rng.uniform(0, 640, bad.sum())
    v[bad] = rng.uniform(0, 480, bad.sum())
    fr["un_xy"][:] = np.stack([u, v], 1).astype(np.float32)
    st = rng.random(n_pts) < stereo
    fr["uright"][:] = np.where(st, ur, -1).astype(np.float32)
    fr["pt_ref"][:] = np.where(rng.random(n_pts) < null_frac, -1, rng.permutation(n_pts)).astype(np.int32)
    # pt_ref is a permutation: keypoint i sees point pt_ref[i]; re-derive its observation from that point
    ok = fr["pt_ref"] >= 0
    perm = np.where(ok, fr["pt_ref"], 0)
    fr["xyz"][perm[ok]] = pw[ok].astype(np.float32)
    fr["outlier"][:] = rng.integers(0, 2, n_pts)                          # entries without an edge keep this
    for i in range(n_lines):
        zz = rng.uniform(1.0, 5.0, 2)
        a = np.array([(rng.uniform(20, 620) - CX) / FX * zz[0], (rng.uniform(20, 460) - CY) / FY * zz[0], zz[0]])
        b = np.array([(rng.uniform(20, 620) - CX) / FX * zz[1], (rng.uniform(20, 460) - CY) / FY * zz[1], zz[1]])
        pa = np.array([a[0] / a[2] * FX + CX, a[1] / a[2] * FY + CY, 1.0])
        pb = np.array([b[0] / b[2] * FX + CX, b[1] / b[2] * FY + CY, 1.0])
        pa[:2] += rng.normal(size=2) * noise
        pb[:2] += rng.normal(size=2) * noise
        if rng.random() < line_outliers:
            pa[:2] += rng.uniform(30, 60, 2)
        l = np.cross(pa, pb)
        fr["line_fn"][i] = l / math.hypot(l[0], l[1])
        fr["line_xyz"][i] = np.concatenate([(a - t) @ R, (b - t) @ R])
        fr["line_has"][i] = 1 if rng.random() > null_frac else 0
    fr["line_outlier"][:] = rng.integers(0, 2, n_lines)
    for i in range(n_planes):
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        d = rng.uniform(0.5, 4.0)
        nw = R.T @ n                                                       # camera plane n.x + d = 0 -> world normal, distance
        dw = d + t @ n
        cam = np.concatenate([n + rng.normal(size=3) * 0.01 * (noise > 0), [d + rng.normal() * 0.01 * (noise > 0)]])
        fr["plane_coef"][i] = cam.astype(np.float32) * (1 if rng.random() < 0.5 else -1)
        fr["plane_w"][i] = np.concatenate([nw, [dw]]).astype(np.float32) * (1 if rng.random() < 0.5 else -1)
        fr["par_w"][i] = np.concatenate([nw, [dw + rng.uniform(0.5, 2)]]).astype(np.float32)
        perp = np.cross(nw, rng.normal(size=3))
        perp /= np.linalg.norm(perp)
        fr["ver_w"][i] = np.concatenate([perp, [rng.uniform(0.5, 3)]]).astype(np.float32)
        fr["plane_has"][i] = 1
        fr["par_has"][i] = 1 if par else 0
        fr["ver_has"][i] = 1 if ver else 0
    for k in ("plane_outlier", "par_outlier", "ver_outlier"):
        fr[k][:] = rng.integers(0, 2, n_planes)
    R0 = rot(rng.normal(size=3), rot_deg) @ R
    t0 = t + rng.normal(size=3) / math.sqrt(3) * trans
    fr["Tcw"][:] = tcw12(R0, t0)
    if xcap is not None:
        scatter(fr, xcap, seed)
    if margin is not None:
        check_margin(fr, c, margin)
    return fr, R, t


def scatter(fr, xcap, seed):
    """Moves fr's xyz rows to distinct slots of an xcap-row xyz (the last keypoint's point to slot xcap - 1) and rewrites pt_ref; the other
    rows are filler points nobody references.  Draws from its own generator, so the rest of the scene is unchanged."""
    n = len(fr["xyz"])
    assert n < xcap
    rng = np.random.default_rng(seed + 104729)
    slot = rng.choice(xcap - 1, n, replace=False)
    ok = fr["pt_ref"] >= 0
    if ok.any():
        slot[fr["pt_ref"][ok][-1]] = xcap - 1
    xyz = rng.normal(0, 3, (xcap, 3)).astype(np.float32)
    xyz[slot] = fr["xyz"]
    fr["pt_ref"][ok] = slot[fr["pt_ref"][ok]]
    fr["xyz"] = xyz


def check_margin(fr, c, margin=1e-4):
    rows = []
    pm.pose_optimization(fr, c, rows)
    for kind, idx, x2, th in rows:
        assert abs(x2 - th) > margin * th, ("chi2 too close to its threshold", kind, idx, x2, th)

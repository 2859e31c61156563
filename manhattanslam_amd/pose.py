"""Host mirror of Optimizer::PoseOptimization (reference src/Optimizer.cc:53-590) through the C ABI (msl_pose_optimize[_batch]) for a batch
of independent frames.  A frame is a dict of numpy arrays -- the per-frame inputs of include/msl.h, named as in tests/pose_model.py:
  octave (N,) i32, un_xy (N,2) f32, uright (N,) f32, pt_ref (N,) i32 (-1 = no MapPoint), xyz (X,3) f32, outlier (N,) u8
  line_fn (NL,3) f64, line_xyz (NL,6) f64, line_has (NL,) u8, line_outlier (NL,) u8
  plane_coef (M,4) f32, plane_w / par_w / ver_w (M,4) f32, plane_has / par_has / ver_has (M,) u8,
  plane_outlier / par_outlier / ver_outlier (M,) u8, Tcw (12,) f32 (rows 0-2 of mTcw)."""
import numpy as np

from ._lib import KEYPOINT_DTYPE, MSL_MEM_HOST, POSE_PARAMS_DTYPE, check, lib, ptr

KINDS = ("plane", "par", "ver")


def pose_params(c):
    """msl_pose_params from the constants dict of tests/pose_scenes.params (fx .. bf, inv_level_sigma2 = mvInvLevelSigma2, and the eight
    Optimizer constructor values angleInfo, disInfo, parInfo, verInfo, planeChi, planeChiVP, aTh, parTh)."""
    p = np.zeros(1, POSE_PARAMS_DTYPE)
    for k in ("fx", "fy", "cx", "cy", "bf"):
        p[k] = c[k]
    p["nlevels"] = len(c["inv_level_sigma2"])
    p["inv_level_sigma2"][0, :len(c["inv_level_sigma2"])] = c["inv_level_sigma2"]
    for k, n in (("angle_info", "angleInfo"), ("dis_info", "disInfo"), ("par_info", "parInfo"), ("ver_info", "verInfo"),
                 ("plane_chi", "planeChi"), ("plane_chi_vp", "planeChiVP"), ("a_th", "aTh"), ("par_th", "parTh")):
        p[k] = c[n]
    return p


def pack(frames, cap=None, xcap=None, lcap=None, pcap=None):
    """Packs per-frame dicts into msl_pose_optimize's [frames][cap] ... arrays.  Returns (caps, inputs in ABI order kps .. Tcw,
    in/out arrays (outlier, line_outlier, plane_outlier))."""
    F = len(frames)
    cap = cap or max(max(len(f["pt_ref"]) for f in frames), 1)
    xcap = xcap or max(max(len(f["xyz"]) for f in frames), 1)
    lcap = lcap or max(max(len(f["line_has"]) for f in frames), 1)
    pcap = pcap or max(max(len(f["plane_coef"]) for f in frames), 1)
    kps = np.zeros((F, cap), KEYPOINT_DTYPE)
    un = np.zeros((F, cap, 2), np.float32); ur = np.full((F, cap), -1, np.float32); ref = np.full((F, cap), -1, np.int32)
    nk = np.zeros(F, np.int32); xyz = np.zeros((F, xcap, 3), np.float32)
    lfn = np.zeros((F, lcap, 3)); lxyz = np.zeros((F, lcap, 6)); lhas = np.zeros((F, lcap), np.uint8); nl = np.zeros(F, np.int32)
    pc = np.zeros((F, pcap, 4), np.float32); pw = np.zeros((F, pcap, 3, 4), np.float32); phas = np.zeros((F, pcap), np.uint8)
    npl = np.zeros(F, np.int32); T = np.zeros((F, 12), np.float32)
    out = np.zeros((F, cap), np.uint8); lout = np.zeros((F, lcap), np.uint8); pout = np.zeros((F, pcap, 3), np.uint8)
    for f, fr in enumerate(frames):
        n, x, l, m = len(fr["pt_ref"]), len(fr["xyz"]), len(fr["line_has"]), len(fr["plane_coef"])
        kps["octave"][f, :n] = fr["octave"]; un[f, :n] = fr["un_xy"]; ur[f, :n] = fr["uright"]; ref[f, :n] = fr["pt_ref"]; nk[f] = n
        xyz[f, :x] = fr["xyz"]; out[f, :n] = fr["outlier"]
        lfn[f, :l] = fr["line_fn"]; lxyz[f, :l] = fr["line_xyz"]; lhas[f, :l] = fr["line_has"]; lout[f, :l] = fr["line_outlier"]; nl[f] = l
        pc[f, :m] = fr["plane_coef"]; npl[f] = m
        for s, k in enumerate(KINDS):
            pw[f, :m, s] = fr[k + "_w"]
            phas[f, :m] |= (np.asarray(fr[k + "_has"], np.uint8) != 0).astype(np.uint8) << s
            pout[f, :m, s] = fr[k + "_outlier"]
        T[f] = fr["Tcw"]
    return (cap, xcap, lcap, pcap), [kps, un, ur, ref, nk, xyz, lfn, lxyz, lhas, nl, pc, pw, phas, npl, T], [out, lout, pout]


def unpack(frames, io, Tcw_out, n_good):
    """Per frame (n_good, Tcw_out (12,) f32, outlier dict with the keys of the frame dicts)."""
    out, lout, pout = io
    res = []
    for f, fr in enumerate(frames):
        n, l, m = len(fr["pt_ref"]), len(fr["line_has"]), len(fr["plane_coef"])
        d = {"outlier": out[f, :n].copy(), "line_outlier": lout[f, :l].copy()}
        for s, k in enumerate(KINDS):
            d[k + "_outlier"] = pout[f, :m, s].copy()
        res.append((int(n_good[f]), Tcw_out[f].copy(), d))
    return res


def pose_optimization_batch(params, frames, device=0, handle=None, caps=None):
    """Optimizer::PoseOptimization for a batch of frames (host arrays, synchronous).  params: a msl_pose_params record (pose_params).
    Returns unpack(...): per frame (n_good, Tcw_out, outlier arrays)."""
    (cap, xcap, lcap, pcap), arrays, io = pack(frames, *(caps or ()))
    F = len(frames)
    Tout = np.zeros((F, 12), np.float32)
    ng = np.zeros(F, np.int32)
    args = [F, cap, xcap, lcap, pcap, ptr(params)] + [ptr(a) for a in arrays] + [MSL_MEM_HOST] + [ptr(a) for a in io] + \
        [ptr(Tout), ptr(ng), MSL_MEM_HOST]
    if handle is not None:
        check(lib.msl_pose_optimize(handle.h, *args), "msl_pose_optimize")
    else:
        check(lib.msl_pose_optimize_batch(device, *args), "msl_pose_optimize_batch")
    return unpack(frames, io, Tout, ng)


def pose_optimization_device(handle, params, n_frames, caps, arrays, io, Tcw_out, n_good):
    """The device form on a match.Matcher handle: arrays (kps .. Tcw, pack's order), io (outlier, line_outlier, plane_outlier, updated in
    place), Tcw_out and n_good are torch tensors on the handle's device.  Asynchronous on the handle's stream (handle.sync())."""
    cap, xcap, lcap, pcap = caps
    check(lib.msl_pose_optimize(handle.h, n_frames, cap, xcap, lcap, pcap, ptr(params), *[ptr(a) for a in arrays], 1,
                                *[ptr(a) for a in io], ptr(Tcw_out), ptr(n_good), 1), "msl_pose_optimize")

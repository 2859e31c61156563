"""Host mirror of Optimizer::PoseOptimization (reference src/Optimizer.cc:53-590) and of Optimizer::TranslationOptimization (:592-1009,
Manhattan mode) through the C ABI (msl_pose_optimize[_batch], msl_pose_optimize_translation[_batch]) for a batch of independent frames.  A frame is a dict of numpy arrays -- the per-frame inputs of include/msl.h, named as in tests/pose_model.py:
  octave (N,) i32, un_xy (N,2) f32, uright (N,) f32, pt_ref (N,) i32 (-1 = no MapPoint), xyz (X,3) f32, outlier (N,) u8
  line_fn (NL,3) f64, line_xyz (NL,6) f64, line_has (NL,) u8, line_outlier (NL,) u8
  plane_coef (M,4) f32, plane_w / par_w / ver_w (M,4) f32, plane_has / par_has / ver_has (M,) u8,
  plane_outlier / par_outlier / ver_outlier (M,) u8, Tcw (12,) f32 (rows 0-2 of mTcw)."""
import numpy as np

from ._lib import KEYPOINT_DTYPE, MSL_MEM_HOST, POSE_PARAMS_DTYPE, call, check, lib, pad, ptr

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
    kps["octave"] = pad(frames, "octave", cap, np.int32)
    phas = np.zeros((F, pcap), np.uint8)
    for f, fr in enumerate(frames):
        for s, k in enumerate(KINDS):
            phas[f, :len(fr["plane_coef"])] |= (np.asarray(fr[k + "_has"], np.uint8) != 0).astype(np.uint8) << s
    count = lambda key: np.array([len(fr[key]) for fr in frames], np.int32)
    kinds = lambda suffix, dtype, shape=(): np.stack([pad(frames, k + suffix, pcap, dtype, shape=shape) for k in KINDS], 2)   # [frames][pcap][3 ...]
    inputs = [kps, pad(frames, "un_xy", cap, np.float32, shape=(2,)), pad(frames, "uright", cap, np.float32, -1),
              pad(frames, "pt_ref", cap, np.int32, -1), count("pt_ref"), pad(frames, "xyz", xcap, np.float32, shape=(3,)),
              pad(frames, "line_fn", lcap, np.float64, shape=(3,)), pad(frames, "line_xyz", lcap, np.float64, shape=(6,)),
              pad(frames, "line_has", lcap, np.uint8), count("line_has"),
              pad(frames, "plane_coef", pcap, np.float32, shape=(4,)), kinds("_w", np.float32, (4,)), phas, count("plane_coef"),
              np.array([fr["Tcw"] for fr in frames], np.float32)]
    io = [pad(frames, "outlier", cap, np.uint8), pad(frames, "line_outlier", lcap, np.uint8), kinds("_outlier", np.uint8)]
    return (cap, xcap, lcap, pcap), inputs, io


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
    call("msl_pose_optimize", handle, device, F, cap, xcap, lcap, pcap, ptr(params), *[ptr(a) for a in arrays], MSL_MEM_HOST,
         *[ptr(a) for a in io], ptr(Tout), ptr(ng), MSL_MEM_HOST)
    return unpack(frames, io, Tout, ng)


def pose_optimization_device(handle, params, n_frames, caps, arrays, io, Tcw_out, n_good):
    """The device form on a match.Matcher handle: arrays (kps .. Tcw, pack's order), io (outlier, line_outlier, plane_outlier, updated in
    place), Tcw_out and n_good are torch tensors on the handle's device.  Asynchronous on the handle's stream (handle.sync())."""
    cap, xcap, lcap, pcap = caps
    check(lib.msl_pose_optimize(handle.h, n_frames, cap, xcap, lcap, pcap, ptr(params), *[ptr(a) for a in arrays], 1,
                                *[ptr(a) for a in io], ptr(Tcw_out), ptr(n_good), 1), "msl_pose_optimize")


def _rcw(rcw, n_frames):
    """None, or the Manhattan rotations as a contiguous (n_frames, 9) float32 array (row-major 3 x 3 per frame)."""
    if rcw is None:
        return None
    return np.ascontiguousarray(np.asarray(rcw, np.float32).reshape(n_frames, 9))


def translation_optimization_batch(params, frames, rcw=None, device=0, handle=None, caps=None):
    """Optimizer::TranslationOptimization for a batch of frames (host arrays, synchronous).  rcw: None (each frame's Tcw is used as given)
    or the frames' manhattanRcw, (n_frames, 3, 3) or (n_frames, 9) float32, written into Tcw's rotation block first (src/Tracking.cc:974).
    Only plane_has / plane_w / plane_outlier of the mvpMapPlanes kind are used.  Returns unpack(...) as pose_optimization_batch does."""
    (cap, xcap, lcap, pcap), arrays, io = pack(frames, *(caps or ()))
    F = len(frames)
    r = _rcw(rcw, F)
    Tout = np.zeros((F, 12), np.float32)
    ng = np.zeros(F, np.int32)
    call("msl_pose_optimize_translation", handle, device, F, cap, xcap, lcap, pcap, ptr(params), *[ptr(a) for a in arrays],
         ptr(r), MSL_MEM_HOST, *[ptr(a) for a in io], ptr(Tout), ptr(ng), MSL_MEM_HOST)
    return unpack(frames, io, Tout, ng)


def translation_optimization_device(handle, params, n_frames, caps, arrays, io, Tcw_out, n_good, rcw=None):
    """The device form on a match.Matcher handle, as pose_optimization_device; rcw is None or a (n_frames, 9) float32 tensor on the
    handle's device.  Asynchronous on the handle's stream (handle.sync())."""
    cap, xcap, lcap, pcap = caps
    check(lib.msl_pose_optimize_translation(handle.h, n_frames, cap, xcap, lcap, pcap, ptr(params), *[ptr(a) for a in arrays],
                                            ptr(rcw), 1, *[ptr(a) for a in io], ptr(Tcw_out), ptr(n_good), 1),
          "msl_pose_optimize_translation")

"""Host mirror of the PnP step of Tracking::Relocalization (reference src/Tracking.cc:1960-2000) through the C ABI: PnPsolver
(src/PnPsolver.cc) -- SetRansacParameters and one iterate() call on a fresh solver -- for a batch of independent (frame, candidate keyframe)
pairs (pnp_ransac), and the per-hypothesis stage of the last call (debug_hypotheses)."""
import numpy as np

from ._lib import KEYPOINT_DTYPE, MSL_MEM_DEVICE, MSL_MEM_HOST, PNP_PARAMS_DTYPE, call, check, lib, pad, ptr


def pnp_params(fx, fy, cx, cy, level_sigma2, probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5, th2=5.991,
               n_iterations=5):
    """msl_pnp_params: the camera, Frame::mvLevelSigma2, the arguments of SetRansacParameters (defaults: Tracking's) and of iterate()."""
    p = np.zeros(1, PNP_PARAMS_DTYPE)
    p["fx"], p["fy"], p["cx"], p["cy"] = fx, fy, cx, cy
    ls = np.asarray(level_sigma2, np.float32).reshape(-1)[:16]
    p["nlevels"] = len(ls)
    p["level_sigma2"][0, :len(ls)] = ls
    p["probability"], p["min_inliers"], p["max_iterations"], p["min_set"] = probability, min_inliers, max_iterations, min_set
    p["epsilon"], p["th2"], p["n_iterations"] = epsilon, th2, n_iterations
    return p


def pack_pnp(pairs, cap=None, kcap=None):
    """Packs per-pair dicts into msl_pnp_ransac's [pairs][cap] / [pairs][kcap] arrays (its argument order, kps .. seed).
       pair: octave (N,) i32 (or kps, KEYPOINT_DTYPE), un_xy (N,2) f32, match (N,) i32, xyz (M,3) f32, seed"""
    cap = cap or max(max(len(p["match"]) for p in pairs), 1)
    kcap = kcap or max(max(len(p["xyz"]) for p in pairs), 1)
    kps = np.zeros((len(pairs), cap), KEYPOINT_DTYPE)
    for f, p in enumerate(pairs):
        if "kps" in p:
            kps[f, :len(p["kps"])] = p["kps"]
        else:
            kps["octave"][f, :len(p["octave"])] = p["octave"]
    return cap, kcap, [kps, pad(pairs, "un_xy", cap, np.float32, shape=(2,)), pad(pairs, "match", cap, np.int32, fill=-1),
                       np.array([len(p["match"]) for p in pairs], np.int32), pad(pairs, "xyz", kcap, np.float32, shape=(3,)),
                       np.array([int(p["seed"]) & 0xFFFFFFFF for p in pairs], np.uint32)]


def pnp_ransac(params, pairs, device=0, handle=None, cap=None, kcap=None):
    """One PnPsolver::iterate(n_iterations) on a fresh solver for every pair (host arrays, synchronous); see pack_pnp.
    Returns (Tcw (B,3,4) f32, inlier: per pair (N,) u8, pt_ref: per pair (N,) i32, n_inliers (B,), status (B,): 0 none, 1 refined, 2 best)."""
    cap, kcap, arrays = pack_pnp(pairs, cap, kcap)
    B = len(pairs)
    Tcw = np.zeros((B, 3, 4), np.float32); inl = np.zeros((B, cap), np.uint8); ref = np.zeros((B, cap), np.int32)
    ni = np.zeros(B, np.int32); st = np.zeros(B, np.int32)
    call("msl_pnp_ransac", handle, device, B, cap, kcap, ptr(params), *[ptr(a) for a in arrays], MSL_MEM_HOST, ptr(Tcw), ptr(inl), ptr(ref),
         ptr(ni), ptr(st), MSL_MEM_HOST)
    n = arrays[3]
    return Tcw, [inl[f, :n[f]].copy() for f in range(B)], [ref[f, :n[f]].copy() for f in range(B)], ni, st


def pnp_ransac_device(handle, params, n_pairs, cap, kcap, arrays, Tcw_out, inlier, pt_ref_out, n_inliers, status):
    """Device-resident inputs and outputs (torch tensors / device pointers in msl.h's argument order, kps .. seed) on a match.Matcher:
    asynchronous on the handle's stream."""
    check(lib.msl_pnp_ransac(handle.h, n_pairs, cap, kcap, ptr(params), *[ptr(a) for a in arrays], MSL_MEM_DEVICE, ptr(Tcw_out), ptr(inlier),
                             ptr(pt_ref_out), ptr(n_inliers), ptr(status), MSL_MEM_DEVICE), "msl_pnp_ransac")


def debug_hypotheses(handle, pair, k_cap=1024):
    """The per-hypothesis stage of the last pnp call on a match.Matcher: (R (K,3,3) f64, t (K,3) f64, branch (K,), count (K,))."""
    R = np.zeros((k_cap, 3, 3)); t = np.zeros((k_cap, 3)); br = np.zeros(k_cap, np.int32); cnt = np.zeros(k_cap, np.int32)
    n = np.zeros(1, np.int32)
    check(lib.msl_pnp_debug_hypotheses(handle.h, pair, k_cap, ptr(R), ptr(t), ptr(br), ptr(cnt), ptr(n)), "msl_pnp_debug_hypotheses")
    k = min(int(n[0]), k_cap)
    return R[:k], t[:k], br[:k], cnt[:k]


__all__ = ["pnp_params", "pack_pnp", "pnp_ransac", "pnp_ransac_device", "debug_hypotheses"]

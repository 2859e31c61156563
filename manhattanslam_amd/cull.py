"""Host mirror of the cullings of LocalMapping::Run through the C ABI: LocalMapping::KeyFrameCulling (reference src/LocalMapping.cc:704-759)
as cull_keyframes, for a batch of independent items over one map, and the elementwise verdict of MapPointCulling / MapLineCulling /
MapPlaneCulling (:227-301) as cull_recent.  Every function takes the arrays under msl.h's names (numpy arrays for host memory, torch
tensors or anything with data_ptr() for device memory) and writes the outputs it is given; with device memory on a match.Matcher the call
is asynchronous on the handle's stream."""
import numpy as np

from ._lib import MSL_MEM_DEVICE, MSL_MEM_HOST, RECORDS, call, ptr

CULL_PARAMS_DTYPE = RECORDS["msl_cull_params"]
assert CULL_PARAMS_DTYPE.itemsize == 4
KEPT, CULLED, ORIGIN, NOT_ERASE, ABSENT = 1, 2, 3, 4, 5               # MSL_CULL_*
RATIO_FLOAT, RATIO_INT = 0, 1                                         # MSL_RATIO_*
RECENT_KEEP, RECENT_ERASE_BAD, RECENT_CULL_RATIO, RECENT_CULL_OBS, RECENT_RETIRE, RECENT_INVALID = range(6)   # MSL_RECENT_*
KF_NOT_BAD, KF_NOT_ERASE = 1, 2                                       # kf_flags bits
MAX_TAB, MAX_CAP, MAX_PTS, MAX_ITEMS, MAX_RECENT = 4096, 8192, 1 << 20, 4096, 1 << 20
KF_IN_KEYS = ("kps_un", "uright", "depth", "held_id", "n_kps", "kf_flags", "pt_flags", "pt_nobs", "obs_off", "obs_kf", "obs_idx", "cand", "n_cand")
KF_OUT_KEYS = ("n_mps", "n_redundant", "n_gone", "status")
RECENT_IN_KEYS = ("found", "visible", "first_kf_id", "nobs", "flags")


def cull_params(th_depth):
    """msl_cull_params from mThDepth."""
    p = np.zeros(1, CULL_PARAMS_DTYPE)
    p["th_depth"] = th_depth
    return p


def keyframes_outputs(n_items, ccap, zeros=np.zeros):
    """The output arrays of one msl_cull_keyframes call, in msl.h's order (zeros(shape, dtype) allocates)."""
    return dict(n_mps=zeros((n_items, ccap), np.int32), n_redundant=zeros((n_items, ccap), np.int32), n_gone=zeros((n_items, ccap), np.int32),
                status=zeros((n_items, ccap), np.uint8))


def cull_keyframes(params, n_tab, cap, n_pts, n_items, n_obs_total, ccap, origin, ins, out, mem=MSL_MEM_HOST, device=0, handle=None):
    """msl_cull_keyframes: `params` from cull_params (always host memory), `ins` keyed by KF_IN_KEYS, `out` by KF_OUT_KEYS; both in `mem`
    memory.  origin: the table index of the keyframe with mnId == 0, or -1.  Returns out."""
    call("msl_cull_keyframes", handle, device, n_tab, cap, n_pts, n_items, n_obs_total, ccap, origin, ptr(params),
         *[ptr(ins.get(k)) for k in KF_IN_KEYS], mem, *[ptr(out.get(k)) for k in KF_OUT_KEYS], mem)
    return out


def cull_keyframes_device(handle, params, n_tab, cap, n_pts, n_items, n_obs_total, ccap, origin, ins, out):
    """Device-resident inputs and outputs on a match.Matcher: asynchronous on the handle's stream."""
    return cull_keyframes(params, n_tab, cap, n_pts, n_items, n_obs_total, ccap, origin, ins, out, MSL_MEM_DEVICE, handle=handle)


def cull_recent(n, cur_kf_id, th_obs, ratio_form, ins, verdict, mem=MSL_MEM_HOST, device=0, handle=None):
    """msl_cull_recent: `ins` keyed by RECENT_IN_KEYS and `verdict` (n,) u8, both in `mem` memory.  Returns verdict."""
    call("msl_cull_recent", handle, device, n, cur_kf_id, th_obs, ratio_form, *[ptr(ins.get(k)) for k in RECENT_IN_KEYS], mem, ptr(verdict), mem)
    return verdict


def cull_recent_device(handle, n, cur_kf_id, th_obs, ratio_form, ins, verdict):
    """Device-resident inputs and output on a match.Matcher: asynchronous on the handle's stream."""
    return cull_recent(n, cur_kf_id, th_obs, ratio_form, ins, verdict, MSL_MEM_DEVICE, handle=handle)


__all__ = ["cull_params", "keyframes_outputs", "cull_keyframes", "cull_keyframes_device", "cull_recent", "cull_recent_device", "CULL_PARAMS_DTYPE",
           "KF_IN_KEYS", "KF_OUT_KEYS", "RECENT_IN_KEYS"]

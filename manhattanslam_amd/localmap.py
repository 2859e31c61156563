"""Host mirror of Tracking::UpdateLocalMap (reference src/Tracking.cc:1754-1764) through the C ABI, for a batch of frames over one map:
UpdateLocalKeyFrames (:1813-1907) as local_keyframes, UpdateLocalPoints (:1789-1810) and UpdateLocalLines (:1766-1787), each with the first
loop of SearchLocalPoints / SearchLocalLines and the gather of the table rows, as local_points and local_lines.  Every function takes the
arrays under msl.h's names (numpy arrays for host memory, torch tensors or anything with data_ptr() for device memory) and writes the
outputs it is given; with device memory on a match.Matcher the call is asynchronous on the handle's stream."""
import numpy as np

from ._lib import MSL_MEM_DEVICE, MSL_MEM_HOST, call, check, lib, ptr

NO_VOTES = 1                                                          # MSL_LOCALMAP_NO_VOTES
MAX_TAB, MAX_CAP, MAX_KLCAP, MAX_PTS, MAX_LINES, MAX_MCAP = 4096, 8192, 256, 1 << 20, 1 << 20, 32768
LOCAL_KF_STOP, BEST_COVIS = 80, 10                                    # the second loop's stop, GetBestCovisibilityKeyFrames(10)
DEFAULT_BUDGET = 256 << 20
KF_IN_KEYS = ("cur_held", "n_cur", "pt_flags", "obs_off", "obs_kf", "kf_flags", "conn", "n_conn", "parent", "prev_kf", "n_prev")
KF_OUT_KEYS = ("votes", "local_kf", "n_local_kf", "ref_kf", "cur_cleared", "status")
POINT_IN_KEYS = ("local_kf", "n_local_kf", "held_id", "n_kps", "cur_held", "n_cur", "pt_xyz", "pt_normal", "pt_dist", "pt_desc", "pt_flags", "pt_nobs")
POINT_OUT_KEYS = ("local_id", "n_local", "mp_xyz", "mp_normal", "mp_dist", "mp_desc", "mp_flags", "cur_flags")
LINE_IN_KEYS = ("local_kf", "n_local_kf", "lheld_id", "n_kl", "cur_lheld", "n_cur_lines", "ln_xyz", "ln_normal", "ln_dist", "ln_desc", "ln_flags", "ln_nobs")
LINE_OUT_KEYS = ("local_line_id", "n_local_lines", "ml_xyz", "ml_normal", "ml_dist", "ml_desc", "ml_flags", "cur_line_flags")


def keyframes_outputs(n_frames, cap, n_tab, zeros=np.zeros):
    """The output arrays of one msl_local_keyframes call, in msl.h's order (zeros(shape, dtype) allocates)."""
    F = n_frames
    return dict(votes=zeros((F, n_tab), np.int32), local_kf=zeros((F, n_tab), np.int32), n_local_kf=zeros((F,), np.int32),
                ref_kf=zeros((F,), np.int32), cur_cleared=zeros((F, cap), np.uint8), status=zeros((F,), np.uint8))


def points_outputs(n_frames, cap, mcap, zeros=np.zeros):
    """The output arrays of one msl_local_points call: what msl_match_local_points reads, plus local_id."""
    F = n_frames
    return dict(local_id=zeros((F, mcap), np.int32), n_local=zeros((F,), np.int32), mp_xyz=zeros((F, mcap, 3), np.float32),
                mp_normal=zeros((F, mcap, 3), np.float32), mp_dist=zeros((F, mcap, 2), np.float32), mp_desc=zeros((F, mcap, 32), np.uint8),
                mp_flags=zeros((F, mcap), np.uint8), cur_flags=zeros((F, cap), np.uint8))


def lines_outputs(n_frames, lcap, mlcap, zeros=np.zeros):
    """The output arrays of one msl_local_lines call: what msl_match_local_lines reads, plus local_line_id."""
    F = n_frames
    return dict(local_line_id=zeros((F, mlcap), np.int32), n_local_lines=zeros((F,), np.int32), ml_xyz=zeros((F, mlcap, 6), np.float64),
                ml_normal=zeros((F, mlcap, 3), np.float64), ml_dist=zeros((F, mlcap, 2), np.float32), ml_desc=zeros((F, mlcap, 32), np.uint8),
                ml_flags=zeros((F, mlcap), np.uint8), cur_line_flags=zeros((F, lcap), np.uint8))


def local_keyframes(n_frames, cap, n_tab, n_pts, n_obs_total, ccap, ins, out, mem=MSL_MEM_HOST, device=0, handle=None):
    """msl_local_keyframes: `ins` keyed by KF_IN_KEYS (prev_kf / n_prev absent or None = NULL), `out` by KF_OUT_KEYS; both in `mem` memory.
    Returns out."""
    call("msl_local_keyframes", handle, device, n_frames, cap, n_tab, n_pts, n_obs_total, ccap, *[ptr(ins.get(k)) for k in KF_IN_KEYS], mem,
         *[ptr(out.get(k)) for k in KF_OUT_KEYS], mem)
    return out


def local_points(n_frames, n_tab, cap, n_pts, mcap, ins, out, mem=MSL_MEM_HOST, device=0, handle=None):
    """msl_local_points: `ins` keyed by POINT_IN_KEYS, `out` by POINT_OUT_KEYS; both in `mem` memory.  Returns out."""
    call("msl_local_points", handle, device, n_frames, n_tab, cap, n_pts, mcap, *[ptr(ins.get(k)) for k in POINT_IN_KEYS], mem,
         *[ptr(out.get(k)) for k in POINT_OUT_KEYS], mem)
    return out


def local_lines(n_frames, n_tab, klcap, lcap, n_lines, mlcap, ins, out, mem=MSL_MEM_HOST, device=0, handle=None):
    """msl_local_lines: `ins` keyed by LINE_IN_KEYS, `out` by LINE_OUT_KEYS; both in `mem` memory.  Returns out."""
    call("msl_local_lines", handle, device, n_frames, n_tab, klcap, lcap, n_lines, mlcap, *[ptr(ins.get(k)) for k in LINE_IN_KEYS], mem,
         *[ptr(out.get(k)) for k in LINE_OUT_KEYS], mem)
    return out


def local_keyframes_device(handle, n_frames, cap, n_tab, n_pts, n_obs_total, ccap, ins, out):
    """Device-resident inputs and outputs on a match.Matcher: asynchronous on the handle's stream."""
    return local_keyframes(n_frames, cap, n_tab, n_pts, n_obs_total, ccap, ins, out, MSL_MEM_DEVICE, handle=handle)


def local_points_device(handle, n_frames, n_tab, cap, n_pts, mcap, ins, out):
    """Device-resident inputs and outputs on a match.Matcher: asynchronous on the handle's stream."""
    return local_points(n_frames, n_tab, cap, n_pts, mcap, ins, out, MSL_MEM_DEVICE, handle=handle)


def local_lines_device(handle, n_frames, n_tab, klcap, lcap, n_lines, mlcap, ins, out):
    """Device-resident inputs and outputs on a match.Matcher: asynchronous on the handle's stream."""
    return local_lines(n_frames, n_tab, klcap, lcap, n_lines, mlcap, ins, out, MSL_MEM_DEVICE, handle=handle)


def set_budget(handle, nbytes=DEFAULT_BUDGET):
    """msl_debug_local_map_budget: the bytes of stamps local_points / local_lines keep in flight on a match.Matcher (a test hook: the
    results do not depend on it)."""
    check(lib.msl_debug_local_map_budget(handle.h, nbytes), "msl_debug_local_map_budget")


__all__ = ["keyframes_outputs", "points_outputs", "lines_outputs", "local_keyframes", "local_points", "local_lines", "local_keyframes_device",
           "local_points_device", "local_lines_device", "set_budget", "KF_IN_KEYS", "KF_OUT_KEYS", "POINT_IN_KEYS", "POINT_OUT_KEYS", "LINE_IN_KEYS",
           "LINE_OUT_KEYS"]

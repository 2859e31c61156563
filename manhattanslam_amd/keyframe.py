"""Host mirror of the hand-over from tracking to local mapping through the C ABI: points_3d is the point half of StereoInitialization
(reference src/Tracking.cc:560-572), UpdateLastFrame (:1062-1104) and CreateNewKeyFrame (:1524-1569); keyframe_decision is the tail of
TrackLocalMap (:1365-1430), mbNewPlane (:429-436), "Clean VO matches" (:450-465) and NeedNewKeyFrame (:1433-1508).  Every function takes the
arrays under msl.h's names (numpy arrays for host memory, torch tensors or anything with data_ptr() for device memory) and writes the
outputs it is given; with device memory on a match.Matcher the call is asynchronous on the handle's stream."""
import numpy as np

from ._lib import KEYPOINT_DTYPE, MSL_MEM_DEVICE, MSL_MEM_HOST, RECORDS, call, fill_levels, pad, ptr
from .plane import MAX_PCAP                                           # the planes of a frame: the plane chain's limit

POINT3D_PARAMS_DTYPE = RECORDS["msl_point3d_params"]
KEYFRAME_FRAME_DTYPE = RECORDS["msl_keyframe_frame"]
KEYFRAME_PARAMS_DTYPE = RECORDS["msl_keyframe_params"]
assert POINT3D_PARAMS_DTYPE.itemsize == 92 and KEYFRAME_FRAME_DTYPE.itemsize == 40 and KEYFRAME_PARAMS_DTYPE.itemsize == 16

ALL, KEYFRAME, FRAME = 0, 1, 2                                        # MSL_POINT3D_*
TRACKED_LOCAL_MAP, TRACK_OK, NEW_PLANE = 1, 2, 4                      # MSL_KF_*: msl_keyframe_frame.flags
C1A, C1B, C1C, C2 = 1, 2, 4, 8                                        # MSL_KF_C*: cond
MAX_CAP, MAX_LCAP, MAX_TAB, MAX_PTS, MAX_LINES = 8192, 256, 4096, 1 << 20, 1 << 20
POINT_IN_KEYS = ("kps_un", "depth", "desc", "n_kps", "cur_held", "pt_nobs", "Tcw", "enable", "first_id")
POINT_OUT_KEYS = ("pt_new", "cleared", "new_xyz", "new_normal", "new_dist", "new_desc", "held_out", "new_order", "n_new", "n_walked")
DECISION_IN_KEYS = ("frames", "depth", "n_cur", "cur_held", "outlier", "cur_lheld", "line_outlier", "n_cur_lines", "n_planes", "pt_nobs", "pt_flags",
                    "ln_nobs", "held_id", "n_kps")
DECISION_INOUT_KEYS = ("plane_match", "plane_outlier")
DECISION_OUT_KEYS = ("found_pt", "found_line", "n_inliers", "track_ok", "new_plane", "held_out", "outlier_out", "lheld_out", "line_outlier_out",
                     "counts", "cond", "need_kf")
FRAME_FIELDS = KEYFRAME_FRAME_DTYPE.names


def point3d_params(fx, fy, cx, cy, th_depth, scale_factors, min_points=100):
    """msl_point3d_params: the camera, mThDepth, the 100 of the call sites and mvScaleFactors."""
    p = np.zeros(1, POINT3D_PARAMS_DTYPE)
    p["fx"], p["fy"], p["cx"], p["cy"], p["th_depth"], p["min_points"] = fx, fy, cx, cy, th_depth, min_points
    fill_levels(p, scale_factors=scale_factors)
    return p


def keyframe_params(max_frames, min_frames, th_depth, only_tracking=False):
    """msl_keyframe_params: mMaxFrames, mMinFrames, mThDepth, mbOnlyTracking."""
    p = np.zeros(1, KEYFRAME_PARAMS_DTYPE)
    p["max_frames"], p["min_frames"], p["th_depth"], p["only_tracking"] = max_frames, min_frames, th_depth, int(only_tracking)
    return p


def frame_records(frames):
    """msl_keyframe_frame records from dicts keyed by FRAME_FIELDS (a missing field is 0)."""
    r = np.zeros(len(frames), KEYFRAME_FRAME_DTYPE)
    for f, fr in enumerate(frames):
        for k in FRAME_FIELDS:
            r[k][f] = np.int64(fr.get(k, 0)).astype(np.int32)
    return r


def pack_points(frames, cap=None):
    """Packs per-frame dicts into msl_points_3d's arrays.  frame: kps_un (n,) KEYPOINT_DTYPE, depth (n,) f32, desc (n, 32) u8, Tcw (3, 4) f32,
    cur_held (n,) i32 (-1 = NULL; absent = all NULL).  Returns (cap, dict of arrays named as in msl.h, without pt_nobs / enable / first_id)."""
    cap = cap or max(max(len(f["depth"]) for f in frames), 1)
    fr = [dict(f, cur_held=f.get("cur_held", np.full(len(f["depth"]), -1, np.int32))) for f in frames]
    return cap, dict(kps_un=pad(fr, "kps_un", cap, KEYPOINT_DTYPE), depth=pad(fr, "depth", cap, np.float32), desc=pad(fr, "desc", cap, np.uint8, shape=(32,)),
                     n_kps=np.array([len(f["depth"]) for f in fr], np.int32), cur_held=pad(fr, "cur_held", cap, np.int32, fill=-1),
                     Tcw=np.stack([np.asarray(f["Tcw"], np.float32).reshape(12) for f in fr]))


def points_outputs(n_frames, cap, zeros=np.zeros):
    """The output arrays of one msl_points_3d call, in msl.h's order (zeros(shape, dtype) allocates)."""
    F = n_frames
    return dict(pt_new=zeros((F, cap), np.uint8), cleared=zeros((F, cap), np.uint8), new_xyz=zeros((F, cap, 3), np.float32),
                new_normal=zeros((F, cap, 3), np.float32), new_dist=zeros((F, cap, 2), np.float32), new_desc=zeros((F, cap, 32), np.uint8),
                held_out=zeros((F, cap), np.int32), new_order=zeros((F, cap), np.int32), n_new=zeros((F,), np.int32), n_walked=zeros((F,), np.int32))


def points_3d(params, n_frames, cap, n_pts, mode, ins, out=None, mem=MSL_MEM_HOST, device=0, handle=None):
    """msl_points_3d: `ins` keyed by POINT_IN_KEYS (an absent or None key = NULL), `out` by POINT_OUT_KEYS (allocated on the host when None);
    both in `mem` memory.  Returns out."""
    out = points_outputs(n_frames, cap) if out is None else out
    call("msl_points_3d", handle, device, n_frames, cap, n_pts, mode, ptr(params), *[ptr(ins.get(k)) for k in POINT_IN_KEYS], mem,
         *[ptr(out.get(k)) for k in POINT_OUT_KEYS], mem)
    return out


def points_3d_device(handle, params, n_frames, cap, n_pts, mode, ins, out):
    """Device-resident inputs and outputs on a match.Matcher: asynchronous on the handle's stream."""
    return points_3d(params, n_frames, cap, n_pts, mode, ins, out, MSL_MEM_DEVICE, handle=handle)


def pack_decision(frames, cap=None, lcap=None, pcap=None):
    """Packs per-frame dicts into msl_keyframe_decision's per-frame arrays.  frame: the FRAME_FIELDS, depth (n,), cur_held (n,), outlier (n,),
    cur_lheld (nl,), line_outlier (nl,), plane_match (np, 3), plane_outlier (np, 3).  Returns (cap, lcap, pcap, dict of arrays)."""
    cap = cap or max(max(len(f["depth"]) for f in frames), 1)
    lcap = lcap or max(max(len(f["cur_lheld"]) for f in frames), 1)
    pcap = pcap or max(max(len(f["plane_match"]) for f in frames), 1)
    return cap, lcap, pcap, dict(
        frames=frame_records(frames), depth=pad(frames, "depth", cap, np.float32), n_cur=np.array([len(f["depth"]) for f in frames], np.int32),
        cur_held=pad(frames, "cur_held", cap, np.int32, fill=-1), outlier=pad(frames, "outlier", cap, np.uint8),
        cur_lheld=pad(frames, "cur_lheld", lcap, np.int32, fill=-1), line_outlier=pad(frames, "line_outlier", lcap, np.uint8),
        n_cur_lines=np.array([len(f["cur_lheld"]) for f in frames], np.int32), n_planes=np.array([len(f["plane_match"]) for f in frames], np.int32),
        plane_match=pad(frames, "plane_match", pcap, np.int32, fill=-1, shape=(3,)), plane_outlier=pad(frames, "plane_outlier", pcap, np.uint8, shape=(3,)))


def decision_outputs(n_frames, cap, lcap, zeros=np.zeros):
    """The output arrays of one msl_keyframe_decision call, in msl.h's order."""
    F = n_frames
    return dict(found_pt=zeros((F, cap), np.uint8), found_line=zeros((F, lcap), np.uint8), n_inliers=zeros((F,), np.int32), track_ok=zeros((F,), np.uint8),
                new_plane=zeros((F,), np.uint8), held_out=zeros((F, cap), np.int32), outlier_out=zeros((F, cap), np.uint8),
                lheld_out=zeros((F, lcap), np.int32), line_outlier_out=zeros((F, lcap), np.uint8), counts=zeros((F, 4), np.int32),
                cond=zeros((F,), np.uint8), need_kf=zeros((F,), np.int32))


def keyframe_decision(params, n_frames, cap, lcap, pcap, n_tab, n_pts, n_lines, ins, out=None, mem=MSL_MEM_HOST, device=0, handle=None):
    """msl_keyframe_decision: `ins` keyed by DECISION_IN_KEYS and DECISION_INOUT_KEYS (plane_match / plane_outlier are edited in place), `out`
    by DECISION_OUT_KEYS (allocated on the host when None); all in `mem` memory.  Returns out."""
    out = decision_outputs(n_frames, cap, lcap) if out is None else out
    call("msl_keyframe_decision", handle, device, n_frames, cap, lcap, pcap, n_tab, n_pts, n_lines, ptr(params), *[ptr(ins.get(k)) for k in DECISION_IN_KEYS],
         mem, *[ptr(ins.get(k)) for k in DECISION_INOUT_KEYS], *[ptr(out.get(k)) for k in DECISION_OUT_KEYS], mem)
    return out


def keyframe_decision_device(handle, params, n_frames, cap, lcap, pcap, n_tab, n_pts, n_lines, ins, out):
    """Device-resident inputs and outputs on a match.Matcher: asynchronous on the handle's stream."""
    return keyframe_decision(params, n_frames, cap, lcap, pcap, n_tab, n_pts, n_lines, ins, out, MSL_MEM_DEVICE, handle=handle)


__all__ = ["ALL", "KEYFRAME", "FRAME", "TRACKED_LOCAL_MAP", "TRACK_OK", "NEW_PLANE", "C1A", "C1B", "C1C", "C2", "POINT_IN_KEYS", "POINT_OUT_KEYS",
           "DECISION_IN_KEYS", "DECISION_INOUT_KEYS", "DECISION_OUT_KEYS", "point3d_params", "keyframe_params", "frame_records", "pack_points",
           "points_outputs", "points_3d", "points_3d_device", "pack_decision", "decision_outputs", "keyframe_decision", "keyframe_decision_device"]

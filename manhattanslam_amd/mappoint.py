"""Host mirror of what LocalMapping runs on its map points and keyframe right after the fusion, through the C ABI: MapPoint::
ComputeDistinctiveDescriptors (reference src/MapPoint.cc:210-270) and MapPoint::UpdateNormalAndDepth (:282-322) for a batch of point ids
(refresh_map_points; with REFRESH_DESC alone over a line-descriptor table it is MapLine::ComputeDistinctiveDescriptors), the counting and
ordering of KeyFrame::UpdateConnections (src/KeyFrame.cc:230-299) for a batch of keyframes (covisibility), and the device-memory forms."""
import numpy as np

from ._lib import KEYPOINT_DTYPE, MSL_MEM_DEVICE, MSL_MEM_HOST, REFRESH_PARAMS_DTYPE, call, check, fill_levels, lib, pad, ptr

REFRESH_DESC, REFRESH_NORMAL = 1, 2                                  # `what`
DESC_WRITTEN, NORMAL_WRITTEN, BAD, NO_OBS, NO_LIVE_KF, TOO_MANY, BAD_OCTAVE = 1, 2, 4, 8, 16, 32, 64   # MSL_REFRESH_* status bits
OBS_MAX = 256
MAX_TAB, MAX_CAP, MAX_PTS = 4096, 8192, 1 << 20
TABLE_KEYS = ("kps_un", "desc", "n_kps", "Tcw", "kf_flags")          # the keyframe table msl_refresh_map_points reads
OBS_KEYS = ("obs_off", "obs_kf", "obs_idx")
POINT_KEYS = ("pt_xyz", "pt_flags", "pt_ref")
OUT_KEYS = ("out_desc", "out_normal", "out_dist", "best_obs", "best_median", "status")
ROW_KEYS = ("pt_desc", "pt_normal", "pt_dist")                       # the optional point-table rows
COVIS_KEYS = ("weight", "conn", "conn_w", "n_conn")


def refresh_params(scale_factors):
    """msl_refresh_params from mvScaleFactors."""
    p = np.zeros(1, REFRESH_PARAMS_DTYPE)
    fill_levels(p, scale_factors=scale_factors)
    return p


def pack_table(keyframes, cap=None):
    """Per-keyframe dicts -> the keyframe table.  keyframe: desc (n, 32) u8 and, unless only descriptors are refreshed, kps_un (n,)
    KEYPOINT_DTYPE and Tcw (3, 4) f32; optional bad (bool).  Returns (cap, dict of arrays named as in msl.h)."""
    cap = cap or max(max(len(k["desc"]) for k in keyframes), 1)
    t = dict(desc=pad(keyframes, "desc", cap, np.uint8, shape=(32,)), n_kps=np.array([len(k["desc"]) for k in keyframes], np.int32),
             kf_flags=np.array([0 if k.get("bad") else 1 for k in keyframes], np.uint8), kps_un=None, Tcw=None)
    if "kps_un" in keyframes[0]:
        t["kps_un"] = pad(keyframes, "kps_un", cap, KEYPOINT_DTYPE)
        t["Tcw"] = np.stack([np.asarray(k["Tcw"], np.float32)[:3, :4].reshape(12) for k in keyframes])
    return cap, t


def pack_observations(observations):
    """[[(keyframe table index, keypoint index), ...] per point id, in the map's iteration order] -> dict(obs_off, obs_kf, obs_idx) (the
    two index arrays have at least one element, which no range names)."""
    off = np.zeros(len(observations) + 1, np.int32)
    off[1:] = np.cumsum([len(o) for o in observations])
    flat = [x for o in observations for x in o]
    arr = np.array(flat, np.int32).reshape(-1, 2) if flat else np.zeros((0, 2), np.int32)
    one = lambda v: np.ascontiguousarray(np.concatenate([v, np.zeros(1, np.int32)]) if not len(v) else v)
    return dict(obs_off=off, obs_kf=one(arr[:, 0]), obs_idx=one(arr[:, 1]))


def refresh_outputs(n_items, zeros=np.zeros):
    """The per-item output arrays of one msl_refresh_map_points call, in msl.h's order (zeros(shape, dtype) allocates)."""
    F = n_items
    return dict(out_desc=zeros((F, 32), np.uint8), out_normal=zeros((F, 3), np.float32), out_dist=zeros((F, 2), np.float32),
                best_obs=zeros((F,), np.int32), best_median=zeros((F,), np.int32), status=zeros((F,), np.uint8))


def covisibility_outputs(n_items, n_tab, ccap, zeros=np.zeros):
    """The output arrays of one msl_covisibility call, in msl.h's order."""
    return dict(weight=zeros((n_items, n_tab), np.int32), conn=zeros((n_items, ccap), np.int32), conn_w=zeros((n_items, ccap), np.int32),
                n_conn=zeros((n_items,), np.int32))


def refresh_map_points(params, keyframes, observations, points, ids, what=REFRESH_DESC | REFRESH_NORMAL, rows=None, device=0, handle=None,
                       cap=None):
    """msl_refresh_map_points on host arrays (synchronous).  observations as pack_observations; points: dict(flags (n,) u8 and, unless only
    descriptors are refreshed, xyz (n, 3) f32 and ref (n,) i32); rows: optional dict of the point-table arrays pt_desc / pt_normal /
    pt_dist, written in place at the rows of ids.  Returns a dict of the per-item outputs (OUT_KEYS)."""
    cap, t = pack_table(keyframes, cap)
    o = pack_observations(observations)
    n_pts = len(observations)
    flags = np.ascontiguousarray(points["flags"], np.uint8)
    xyz = np.ascontiguousarray(points["xyz"], np.float32) if points.get("xyz") is not None else None
    ref = np.ascontiguousarray(points["ref"], np.int32) if points.get("ref") is not None else None
    ids = np.ascontiguousarray(ids, np.int32)
    out = refresh_outputs(len(ids))
    rows = rows or {}
    call("msl_refresh_map_points", handle, device, len(keyframes), cap, n_pts, len(ids), int(o["obs_off"][-1]), what, ptr(params),
         *[ptr(t[k]) for k in TABLE_KEYS], *[ptr(o[k]) for k in OBS_KEYS], ptr(xyz), ptr(flags), ptr(ref), ptr(ids), MSL_MEM_HOST,
         *[ptr(out[k]) for k in OUT_KEYS], *[ptr(rows.get(k)) for k in ROW_KEYS], MSL_MEM_HOST)
    return out


def refresh_map_points_device(handle, params, n_tab, cap, n_pts, n_items, n_obs_total, what, table, obs, points, ids, out, rows):
    """Device-resident inputs and outputs (torch tensors / device pointers: `table` keyed by TABLE_KEYS, `obs` by OBS_KEYS, `points` by
    POINT_KEYS, `out` by OUT_KEYS, `rows` by ROW_KEYS, absent or None = NULL) on a match.Matcher: asynchronous on the handle's stream."""
    check(lib.msl_refresh_map_points(handle.h, n_tab, cap, n_pts, n_items, n_obs_total, what, ptr(params), *[ptr(table.get(k)) for k in TABLE_KEYS],
                                     *[ptr(obs[k]) for k in OBS_KEYS], *[ptr(points.get(k)) for k in POINT_KEYS], ptr(ids), MSL_MEM_DEVICE,
                                     *[ptr(out[k]) for k in OUT_KEYS], *[ptr(rows.get(k)) for k in ROW_KEYS], MSL_MEM_DEVICE),
          "msl_refresh_map_points")


def covisibility(keyframes, observations, pt_flags, kf, th=15, ccap=None, device=0, handle=None, cap=None):
    """msl_covisibility on host arrays (synchronous).  keyframes: dicts with held_id (n,) i32, one entry per keypoint; kf: the
    table indices to compute.  Returns a dict of the outputs (COVIS_KEYS)."""
    cap = cap or max(max(len(k["held_id"]) for k in keyframes), 1)
    held = pad(keyframes, "held_id", cap, np.int32, fill=-1)
    n_kps = np.array([len(k["held_id"]) for k in keyframes], np.int32)
    o = pack_observations(observations)
    flags = np.ascontiguousarray(pt_flags, np.uint8)
    kf = np.ascontiguousarray(kf, np.int32)
    ccap = ccap or len(keyframes)
    out = covisibility_outputs(len(kf), len(keyframes), ccap)
    call("msl_covisibility", handle, device, len(keyframes), cap, len(observations), len(kf), int(o["obs_off"][-1]), ccap, th, ptr(held), ptr(n_kps),
         ptr(flags), ptr(o["obs_off"]), ptr(o["obs_kf"]), ptr(kf), MSL_MEM_HOST, *[ptr(out[k]) for k in COVIS_KEYS], MSL_MEM_HOST)
    return out


def covisibility_device(handle, n_tab, cap, n_pts, n_items, n_obs_total, ccap, th, held_id, n_kps, pt_flags, obs_off, obs_kf, kf, out):
    """Device-resident inputs and outputs (`out` keyed by COVIS_KEYS) on a match.Matcher: asynchronous on the handle's stream."""
    check(lib.msl_covisibility(handle.h, n_tab, cap, n_pts, n_items, n_obs_total, ccap, th, ptr(held_id), ptr(n_kps), ptr(pt_flags), ptr(obs_off),
                               ptr(obs_kf), ptr(kf), MSL_MEM_DEVICE, *[ptr(out[k]) for k in COVIS_KEYS], MSL_MEM_DEVICE), "msl_covisibility")


__all__ = ["refresh_params", "pack_table", "pack_observations", "refresh_outputs", "covisibility_outputs", "refresh_map_points",
           "refresh_map_points_device", "covisibility", "covisibility_device", "TABLE_KEYS", "OBS_KEYS", "POINT_KEYS", "OUT_KEYS", "ROW_KEYS",
           "COVIS_KEYS"]

"""Host mirror of the point half of LocalMapping::SearchInNeighbors (reference src/LocalMapping.cc:545-569) through the C ABI: the
de-duplicated candidate list of the target keyframes (fuse_candidates), ORBmatcher::Fuse (src/ORBmatcher.cc:408-546) for a batch of (target
keyframe, candidate list) items from the state on entry (fuse_map_points), the device-memory forms and the projection stage of the last call
(debug_fuse)."""
import numpy as np

from ._lib import FUSE_PARAMS_DTYPE, KEYPOINT_DTYPE, MSL_MEM_DEVICE, MSL_MEM_HOST, call, check, fill_levels, lib, pad, ptr

# MSL_FUSE_*: the exit of the loop body a candidate took
(NULL, BAD, IN_KEYFRAME, BEHIND, OUT_OF_IMAGE, DISTANCE, VIEW_ANGLE, NO_FEATURE, NO_CANDIDATE, ABOVE_TH_LOW, ADDED, REPLACED_BY_HELD, REPLACES_HELD,
 HELD_BAD, UNRESOLVED) = range(15)
MAX_CAP, MAX_TAB, MAX_PTS, MAX_LCAP, MAX_TCAP, MAX_ITEMS = 8192, 4096, 1 << 20, 65536, 64, 4096
TABLE_KEYS = ("kps_un", "uright", "grid_cell", "desc", "n_kps", "Tcw", "held_id")
POINT_KEYS = ("pt_xyz", "pt_normal", "pt_dist", "pt_desc", "pt_flags", "pt_nobs")
OUT_KEYS = ("best_idx", "best_dist", "status", "other", "n_fused")


def fuse_params(fx, fy, cx, cy, bf, min_x, max_x, min_y, max_y, scale_factors, inv_level_sigma2, log_scale_factor, th=3.0, th_low=50):
    """msl_fuse_params; th = 3.0 and th_low = TH_LOW = 50 are the values of both call sites."""
    p = np.zeros(1, FUSE_PARAMS_DTYPE)
    p["fx"], p["fy"], p["cx"], p["cy"], p["bf"] = fx, fy, cx, cy, bf
    p["minX"], p["maxX"], p["minY"], p["maxY"], p["th"] = min_x, max_x, min_y, max_y, th
    fill_levels(p, scale_factors=scale_factors, inv_level_sigma2=inv_level_sigma2)
    p["log_scale_factor"], p["th_low"] = log_scale_factor, th_low
    return p


def pack_table(keyframes, cap=None):
    """Per-keyframe dicts -> the keyframe table.  keyframe: kps_un (n,) KEYPOINT_DTYPE, uright (n,) f32, grid_cell (n,) i32, desc (n, 32) u8,
    held_id (n,) i32, Tcw (3, 4) f32.  Returns (cap, dict of arrays named as in msl.h)."""
    cap = cap or max(max(len(k["kps_un"]) for k in keyframes), 1)
    return cap, dict(kps_un=pad(keyframes, "kps_un", cap, KEYPOINT_DTYPE), uright=pad(keyframes, "uright", cap, np.float32, fill=-1),
                     grid_cell=pad(keyframes, "grid_cell", cap, np.int32, fill=-1), desc=pad(keyframes, "desc", cap, np.uint8, shape=(32,)),
                     n_kps=np.array([len(k["kps_un"]) for k in keyframes], np.int32),
                     Tcw=np.stack([np.asarray(k["Tcw"], np.float32)[:3, :4].reshape(12) for k in keyframes]),
                     held_id=pad(keyframes, "held_id", cap, np.int32, fill=-1))


def pack_points(points):
    """dict(xyz (n, 3), normal (n, 3), dist (n, 2), desc (n, 32), flags (n,), nobs (n,)) -> the point table (at least one row)."""
    n = max(len(points["xyz"]), 1)
    out = dict(pt_xyz=np.zeros((n, 3), np.float32), pt_normal=np.zeros((n, 3), np.float32), pt_dist=np.zeros((n, 2), np.float32),
               pt_desc=np.zeros((n, 32), np.uint8), pt_flags=np.zeros(n, np.uint8), pt_nobs=np.zeros(n, np.int32))
    for k in ("xyz", "normal", "dist", "desc", "flags", "nobs"):
        out["pt_" + k][:len(points[k])] = points[k]
    return n, out


def pack_lists(lists, lcap=None):
    """[[point id or -1, ...], ...] -> (lcap, cand [lists][lcap] (-1 padded), n_cand)."""
    lcap = lcap or max(max((len(l) for l in lists), default=0), 1)
    cand = np.full((max(len(lists), 1), lcap), -1, np.int32)
    for i, l in enumerate(lists):
        cand[i, :len(l)] = l
    n_cand = np.zeros(max(len(lists), 1), np.int32)
    n_cand[:len(lists)] = [len(l) for l in lists]
    return lcap, cand, n_cand


def outputs(n_items, lcap, zeros=np.zeros):
    """The output arrays of one msl_fuse_map_points or msl_fuse_map_lines call, in msl.h's order (zeros(shape, dtype) allocates)."""
    F, L = n_items, lcap
    return dict(best_idx=zeros((F, L), np.int32), best_dist=zeros((F, L), np.int32), status=zeros((F, L), np.uint8), other=zeros((F, L), np.int32),
                n_fused=zeros((F,), np.int32))


def fuse_candidates(keyframes, points, items, device=0, handle=None, cap=None, tcap=None, lcap=None):
    """msl_fuse_candidates on host arrays.  items: [[target table index, ...], ...].  Returns (cand [items][lcap], n_cand)."""
    cap, t = pack_table(keyframes, cap)
    n_pts, p = pack_points(points)
    tcap = tcap or max(max((len(i) for i in items), default=0), 1)
    lcap = lcap or tcap * cap
    targets = np.full((len(items), tcap), -1, np.int32)
    for f, it in enumerate(items):
        targets[f, :len(it)] = it
    n_targets = np.array([len(i) for i in items], np.int32)
    cand = np.zeros((len(items), lcap), np.int32); n_cand = np.zeros(len(items), np.int32)
    call("msl_fuse_candidates", handle, device, len(keyframes), cap, n_pts, len(items), tcap, lcap, ptr(t["held_id"]), ptr(t["n_kps"]),
         ptr(p["pt_flags"]), ptr(targets), ptr(n_targets), MSL_MEM_HOST, ptr(cand), ptr(n_cand), MSL_MEM_HOST)
    return cand, n_cand


def fuse_candidates_device(handle, n_tab, cap, n_pts, n_items, tcap, lcap, held_id, n_kps, pt_flags, targets, n_targets, cand, n_cand):
    """Device-resident inputs and outputs on a match.Matcher: asynchronous on the handle's stream."""
    check(lib.msl_fuse_candidates(handle.h, n_tab, cap, n_pts, n_items, tcap, lcap, ptr(held_id), ptr(n_kps), ptr(pt_flags), ptr(targets),
                                  ptr(n_targets), MSL_MEM_DEVICE, ptr(cand), ptr(n_cand), MSL_MEM_DEVICE), "msl_fuse_candidates")


def fuse_map_points(params, keyframes, points, items, lists, device=0, handle=None, cap=None, lcap=None):
    """msl_fuse_map_points on host arrays (synchronous).  items: [(target table index, list index), ...]; lists as pack_lists.  Returns a
    dict of the outputs (OUT_KEYS)."""
    cap, t = pack_table(keyframes, cap)
    n_pts, p = pack_points(points)
    lcap, cand, n_cand = pack_lists(lists, lcap)
    tgt = np.array([i[0] for i in items], np.int32); lst = np.array([i[1] for i in items], np.int32)
    out = outputs(len(items), lcap)
    call("msl_fuse_map_points", handle, device, len(keyframes), cap, n_pts, len(items), len(cand), lcap, ptr(params), *[ptr(t[k]) for k in TABLE_KEYS],
         *[ptr(p[k]) for k in POINT_KEYS], ptr(tgt), ptr(lst), ptr(cand), ptr(n_cand), MSL_MEM_HOST, *[ptr(out[k]) for k in OUT_KEYS], MSL_MEM_HOST)
    return out


def fuse_map_points_device(handle, params, n_tab, cap, n_pts, n_items, n_lists, lcap, table, points, tgt, lst, cand, n_cand, out):
    """Device-resident inputs and outputs (torch tensors / device pointers: `table` keyed by TABLE_KEYS, `points` by POINT_KEYS, `out` by
    OUT_KEYS) on a match.Matcher: asynchronous on the handle's stream."""
    check(lib.msl_fuse_map_points(handle.h, n_tab, cap, n_pts, n_items, n_lists, lcap, ptr(params), *[ptr(table[k]) for k in TABLE_KEYS],
                                  *[ptr(points[k]) for k in POINT_KEYS], ptr(tgt), ptr(lst), ptr(cand), ptr(n_cand), MSL_MEM_DEVICE,
                                  *[ptr(out[k]) for k in OUT_KEYS], MSL_MEM_DEVICE), "msl_fuse_map_points")


def debug_fuse(handle, item, lcap):
    """One item of the last msl_fuse_map_points call on a match.Matcher (lcap: that call's): dict(u, v, ur (lcap,) f32, level, n_indices
    (lcap,) i32) -- zeros where the candidate left before the value was formed."""
    uvr = np.zeros((lcap, 3), np.float32); ln = np.zeros((lcap, 2), np.int32)
    check(lib.msl_debug_fuse(handle.h, item, ptr(uvr), ptr(ln)), "msl_debug_fuse")
    return dict(u=uvr[:, 0].copy(), v=uvr[:, 1].copy(), ur=uvr[:, 2].copy(), level=ln[:, 0].copy(), n_indices=ln[:, 1].copy())


__all__ = ["fuse_params", "pack_table", "pack_points", "pack_lists", "outputs", "fuse_candidates", "fuse_candidates_device", "fuse_map_points",
           "fuse_map_points_device", "debug_fuse", "TABLE_KEYS", "POINT_KEYS", "OUT_KEYS"]

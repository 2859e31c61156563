"""Host mirror of the line half of LocalMapping::SearchInNeighbors (reference src/LocalMapping.cc:583-618) through the C ABI:
LSDmatcher::Fuse (src/LSDmatcher.cpp:259-382) for a batch of (target keyframe, candidate list) items from the state on entry
(fuse_map_lines), MapLine::UpdateAverageDir (src/MapLine.cpp:262-308) for a batch of line ids (refresh_map_lines), the device-memory forms
and the query stage of the last fusion call (debug_line_fuse).  The candidate list of :589-605 is fuse.fuse_candidates over the line
held_id and flags; MapLine::ComputeDistinctiveDescriptors is mappoint.refresh_map_points with REFRESH_DESC alone."""
import numpy as np

from ._lib import KEYLINE_DTYPE, LINE_FUSE_PARAMS_DTYPE, MSL_MEM_DEVICE, MSL_MEM_HOST, call, check, fill_levels, lib, pad, ptr
from .fuse import outputs, pack_lists
from .mappoint import pack_observations

# MSL_LFUSE_*: the exit of the loop body a candidate took
(NULL, BAD, BEHIND, OUT_OF_IMAGE, DISTANCE, VIEW_ANGLE, NO_FEATURE, NO_CANDIDATE, ABOVE_TH_LOW, ADDED, REPLACED_BY_HELD, REPLACES_HELD, HELD_BAD,
 UNRESOLVED, SELF) = range(15)
INT_MAX = 2 ** 31 - 1                                                  # best_dist of a candidate without a best keyline
MAX_KLCAP, MAX_TAB, MAX_LINES, MAX_LCAP, MAX_ITEMS = 256, 4096, 1 << 20, 65536, 4096
TABLE_KEYS = ("kl", "ldesc", "n_kl", "Tcw", "held_id")
LINE_KEYS = ("ln_xyz", "ln_normal", "ln_dist", "ln_desc", "ln_flags", "ln_nobs")
OUT_KEYS = ("best_idx", "best_dist", "status", "other", "n_fused")
REFRESH_TABLE_KEYS = ("kl", "n_kl", "Tcw")
OBS_KEYS = ("obs_off", "obs_kf", "obs_idx")
REFRESH_LINE_KEYS = ("ln_xyz", "ln_flags", "ln_ref")
REFRESH_OUT_KEYS = ("out_normal", "out_dist", "status")
ROW_KEYS = ("ln_normal", "ln_dist")                                    # the optional line-table rows


def line_fuse_params(fx, fy, cx, cy, min_x, max_x, min_y, max_y, scale_factors, log_scale_factor, th=3.0, th_low=50):
    """msl_line_fuse_params; th = 3.0 and th_low = TH_LOW = 50 are the reference's values."""
    p = np.zeros(1, LINE_FUSE_PARAMS_DTYPE)
    p["fx"], p["fy"], p["cx"], p["cy"] = fx, fy, cx, cy
    p["minX"], p["maxX"], p["minY"], p["maxY"], p["th"] = min_x, max_x, min_y, max_y, th
    fill_levels(p, scale_factors=scale_factors)
    p["log_scale_factor"], p["th_low"] = log_scale_factor, th_low
    return p


def pack_line_table(keyframes, klcap=None):
    """Per-keyframe dicts -> the keyframe line table.  keyframe: kl (n,) KEYLINE_DTYPE, ldesc (n, 32) u8, held_id (n,) i32 (optional),
    Tcw (3, 4) f32.  Returns (klcap, dict of arrays named as in msl.h)."""
    klcap = klcap or max(max(len(k["kl"]) for k in keyframes), 1)
    held = [dict(held_id=k["held_id"] if "held_id" in k else np.full(len(k["kl"]), -1, np.int32)) for k in keyframes]
    return klcap, dict(kl=pad(keyframes, "kl", klcap, KEYLINE_DTYPE), ldesc=pad(keyframes, "ldesc", klcap, np.uint8, shape=(32,)),
                       n_kl=np.array([len(k["kl"]) for k in keyframes], np.int32),
                       Tcw=np.stack([np.asarray(k["Tcw"], np.float32)[:3, :4].reshape(12) for k in keyframes]),
                       held_id=pad(held, "held_id", klcap, np.int32, fill=-1))


def pack_lines(lines):
    """dict(xyz (n, 6) f64, normal (n, 3) f64, dist (n, 2) f32, desc (n, 32), flags (n,), nobs (n,); optional ref (n,)) -> the line table
    (at least one row)."""
    n = max(len(lines["xyz"]), 1)
    out = dict(ln_xyz=np.zeros((n, 6), np.float64), ln_normal=np.zeros((n, 3), np.float64), ln_dist=np.zeros((n, 2), np.float32),
               ln_desc=np.zeros((n, 32), np.uint8), ln_flags=np.zeros(n, np.uint8), ln_nobs=np.zeros(n, np.int32), ln_ref=np.zeros(n, np.int32))
    for k in ("xyz", "normal", "dist", "desc", "flags", "nobs", "ref"):
        if lines.get(k) is not None:
            out["ln_" + k][:len(lines[k])] = lines[k]
    return n, out


def refresh_outputs(n_items, zeros=np.zeros):
    """The per-item output arrays of one msl_refresh_map_lines call, in msl.h's order."""
    return dict(out_normal=zeros((n_items, 3), np.float64), out_dist=zeros((n_items, 2), np.float32), status=zeros((n_items,), np.uint8))


def fuse_map_lines(params, keyframes, lines, items, lists, device=0, handle=None, klcap=None, lcap=None):
    """msl_fuse_map_lines on host arrays (synchronous).  items: [(target table index, list index), ...]; lists as fuse.pack_lists.
    Returns a dict of the outputs (OUT_KEYS)."""
    klcap, t = pack_line_table(keyframes, klcap)
    n_lines, p = pack_lines(lines)
    lcap, cand, n_cand = pack_lists(lists, lcap)
    tgt = np.array([i[0] for i in items], np.int32); lst = np.array([i[1] for i in items], np.int32)
    out = outputs(len(items), lcap)
    call("msl_fuse_map_lines", handle, device, len(keyframes), klcap, n_lines, len(items), len(cand), lcap, ptr(params), *[ptr(t[k]) for k in TABLE_KEYS],
         *[ptr(p[k]) for k in LINE_KEYS], ptr(tgt), ptr(lst), ptr(cand), ptr(n_cand), MSL_MEM_HOST, *[ptr(out[k]) for k in OUT_KEYS], MSL_MEM_HOST)
    return out


def fuse_map_lines_device(handle, params, n_tab, klcap, n_lines, n_items, n_lists, lcap, table, lines, tgt, lst, cand, n_cand, out):
    """Device-resident inputs and outputs (torch tensors / device pointers: `table` keyed by TABLE_KEYS, `lines` by LINE_KEYS, `out` by
    OUT_KEYS) on a match.Matcher: asynchronous on the handle's stream."""
    check(lib.msl_fuse_map_lines(handle.h, n_tab, klcap, n_lines, n_items, n_lists, lcap, ptr(params), *[ptr(table[k]) for k in TABLE_KEYS],
                                 *[ptr(lines[k]) for k in LINE_KEYS], ptr(tgt), ptr(lst), ptr(cand), ptr(n_cand), MSL_MEM_DEVICE,
                                 *[ptr(out[k]) for k in OUT_KEYS], MSL_MEM_DEVICE), "msl_fuse_map_lines")


def refresh_map_lines(params, keyframes, observations, lines, ids, rows=None, device=0, handle=None, klcap=None):
    """msl_refresh_map_lines on host arrays (synchronous).  params: mappoint.refresh_params; observations as mappoint.pack_observations;
    lines: dict(xyz (n, 6) f64, flags (n,) u8, ref (n,) i32); rows: optional dict of the line-table arrays ln_normal / ln_dist, written in
    place at the rows of ids.  Returns a dict of the per-item outputs (REFRESH_OUT_KEYS)."""
    klcap, t = pack_line_table(keyframes, klcap)
    o = pack_observations(observations)
    n_lines = len(observations)
    xyz = np.ascontiguousarray(lines["xyz"], np.float64); flags = np.ascontiguousarray(lines["flags"], np.uint8)
    ref = np.ascontiguousarray(lines["ref"], np.int32); ids = np.ascontiguousarray(ids, np.int32)
    out = refresh_outputs(len(ids))
    rows = rows or {}
    call("msl_refresh_map_lines", handle, device, len(keyframes), klcap, n_lines, len(ids), int(o["obs_off"][-1]), ptr(params),
         *[ptr(t[k]) for k in REFRESH_TABLE_KEYS], *[ptr(o[k]) for k in OBS_KEYS], ptr(xyz), ptr(flags), ptr(ref), ptr(ids), MSL_MEM_HOST,
         *[ptr(out[k]) for k in REFRESH_OUT_KEYS], *[ptr(rows.get(k)) for k in ROW_KEYS], MSL_MEM_HOST)
    return out


def refresh_map_lines_device(handle, params, n_tab, klcap, n_lines, n_items, n_obs_total, table, obs, lines, ids, out, rows):
    """Device-resident inputs and outputs (`table` keyed by REFRESH_TABLE_KEYS, `obs` by OBS_KEYS, `lines` by REFRESH_LINE_KEYS, `out` by
    REFRESH_OUT_KEYS, `rows` by ROW_KEYS, absent or None = NULL) on a match.Matcher: asynchronous on the handle's stream."""
    check(lib.msl_refresh_map_lines(handle.h, n_tab, klcap, n_lines, n_items, n_obs_total, ptr(params), *[ptr(table[k]) for k in REFRESH_TABLE_KEYS],
                                    *[ptr(obs[k]) for k in OBS_KEYS], *[ptr(lines[k]) for k in REFRESH_LINE_KEYS], ptr(ids), MSL_MEM_DEVICE,
                                    *[ptr(out[k]) for k in REFRESH_OUT_KEYS], *[ptr(rows.get(k)) for k in ROW_KEYS], MSL_MEM_DEVICE),
          "msl_refresh_map_lines")


def debug_line_fuse(handle, item, lcap):
    """One item of the last msl_fuse_map_lines call on a match.Matcher (lcap: that call's): dict(u1, v1, u2, v2, radius (lcap,) f32, level,
    n_indices (lcap,) i32) -- zeros where the candidate left before the value was formed."""
    uvr = np.zeros((lcap, 5), np.float32); ln = np.zeros((lcap, 2), np.int32)
    check(lib.msl_debug_line_fuse(handle.h, item, ptr(uvr), ptr(ln)), "msl_debug_line_fuse")
    return dict(u1=uvr[:, 0].copy(), v1=uvr[:, 1].copy(), u2=uvr[:, 2].copy(), v2=uvr[:, 3].copy(), radius=uvr[:, 4].copy(), level=ln[:, 0].copy(),
                n_indices=ln[:, 1].copy())


__all__ = ["line_fuse_params", "pack_line_table", "pack_lines", "outputs", "refresh_outputs", "fuse_map_lines", "fuse_map_lines_device",
           "refresh_map_lines", "refresh_map_lines_device", "debug_line_fuse", "TABLE_KEYS", "LINE_KEYS", "OUT_KEYS", "REFRESH_TABLE_KEYS",
           "OBS_KEYS", "REFRESH_LINE_KEYS", "REFRESH_OUT_KEYS", "ROW_KEYS"]

"""Host mirror of ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th) (reference src/ORBmatcher.cc:547-678) through the
C ABI, for a batch of independent frame pairs, and of the local-map search Tracking::SearchLocalPoints
(src/Tracking.cc:1654-1695: isInFrustum + SearchByProjection(Frame&, vector<MapPoint*>, th)) for a batch of frames, and of the two map-line
searches LSDmatcher::SearchByProjection (src/LSDmatcher.cpp:21-198: the last frame's lines, and Tracking::SearchLocalLines' local map lines)."""
import numpy as np

from ._lib import (KEYLINE_DTYPE, KEYPOINT_DTYPE, LINE_TRACK_DTYPE, LOCAL_MATCH_PARAMS_DTYPE, LOCAL_TRACK_DTYPE, MATCH_PARAMS_DTYPE, MSL_MEM_HOST, call,
                   check, lib, pad, ptr)


def match_params(frame_params, scale_factors, th, check_orientation=True):
    """msl_match_params from the frame's msl_frame_params (fx..cy, bf, image bounds) and the extractor's mvScaleFactors."""
    p = np.zeros(1, MATCH_PARAMS_DTYPE)
    for k in ("fx", "fy", "cx", "cy", "bf", "minX", "maxX", "minY", "maxY"):
        p[k] = frame_params[k][0]
    p["th"] = th
    p["check_orientation"] = 1 if check_orientation else 0
    p["nlevels"] = len(scale_factors)
    p["scale_factors"][0, :len(scale_factors)] = scale_factors
    return p


def local_match_params(frame_params, scale_factors, th, log_scale_factor, view_cos_limit=0.5, nn_ratio=0.8):
    """msl_local_match_params: match_params(...) plus Frame::mfLogScaleFactor, isInFrustum's viewingCosLimit and ORBmatcher's mfNNratio
    (SearchLocalPoints calls isInFrustum(pMP, 0.5) and ORBmatcher(0.8), th = 3, or 5 right after a relocalisation)."""
    p = np.zeros(1, LOCAL_MATCH_PARAMS_DTYPE)
    b = match_params(frame_params, scale_factors, th, False)
    for k in MATCH_PARAMS_DTYPE.names:
        p[k] = b[k]
    p["log_scale_factor"], p["view_cos_limit"], p["nn_ratio"] = log_scale_factor, view_cos_limit, nn_ratio
    return p


def line_match_params(frame_params, scale_factors, th, log_scale_factor, view_cos_limit=0.6, nn_ratio=0.6):
    """msl_line_match_params (the layout of msl_local_match_params): th = 15 for the last-frame search, 1 (5 right after a relocalisation)
    for SearchLocalLines; isInFrustum(pML, 0.6) and LSDmatcher()'s default mfNNratio 0.6."""
    return local_match_params(frame_params, scale_factors, th, log_scale_factor, view_cos_limit, nn_ratio)


class Matcher:
    """One msl_match handle (= one ORBmatcher object, src/ORBmatcher.cc:41): own stream, own cached device buffers."""

    def __init__(self, device=0):
        self.h = lib.msl_match_create(device)
        if not self.h:
            from ._lib import MslError
            raise MslError(lib.msl_last_error().decode())
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            lib.msl_match_destroy(self.h)
            self.h = None

    __del__ = close

    def sync(self):
        check(lib.msl_match_sync(self.h), "msl_match_sync")

    def set_stream(self, hip_stream):
        check(lib.msl_match_set_stream(self.h, hip_stream), "msl_match_set_stream")

    def search_by_projection_batch(self, params, cur, last, Tcw_cur, Tcw_last):
        return search_by_projection_batch(params, cur, last, Tcw_cur, Tcw_last, handle=self)

    def search_by_projection_device(self, params, n_pairs, cap, arrays, match_out, nmatches):
        """Device-resident inputs and outputs (torch tensors / device pointers in msl.h's argument order): asynchronous on the handle's stream."""
        check(lib.msl_match_by_projection(self.h, n_pairs, cap, ptr(params), *[ptr(a) for a in arrays], 1, ptr(match_out), ptr(nmatches), 1), "msl_match_by_projection")

    def search_local_points_batch(self, params, cur, local, Tcw):
        return search_local_points_batch(params, cur, local, Tcw, handle=self)

    def search_local_points_device(self, params, n_frames, cap, mcap, arrays, match_out, n_to_match, nmatches, in_view=None, track=None):
        """Device-resident inputs and outputs (torch tensors / device pointers in msl.h's argument order, cur_kps .. Tcw): asynchronous on
        the handle's stream.  in_view / track may be None."""
        check(lib.msl_match_local_points(self.h, n_frames, cap, mcap, ptr(params), *[ptr(a) for a in arrays], 1, ptr(match_out), ptr(n_to_match),
                                         ptr(nmatches), ptr(in_view), ptr(track), 1), "msl_match_local_points")

    def search_lines_by_projection_batch(self, params, cur, last, Tcw_cur, Tcw_last, **kw):
        return search_lines_by_projection_batch(params, cur, last, Tcw_cur, Tcw_last, handle=self, **kw)

    def search_local_lines_batch(self, params, cur, local, Tcw, **kw):
        return search_local_lines_batch(params, cur, local, Tcw, handle=self, **kw)

    def search_lines_by_projection_device(self, params, n_frames, lcap, llcap, arrays, match_out, nmatches, line_xyz=None, line_has=None):
        """Device-resident inputs and outputs (pack_lines_last's order, cur_kl .. Tcw_last): asynchronous on the handle's stream."""
        check(lib.msl_match_lines_by_projection(self.h, n_frames, lcap, llcap, ptr(params), *[ptr(a) for a in arrays], 1, ptr(match_out),
                                                ptr(nmatches), ptr(line_xyz), ptr(line_has), 1), "msl_match_lines_by_projection")

    def search_local_lines_device(self, params, n_frames, lcap, mlcap, arrays, match_out, n_to_match, nmatches, in_view=None, track=None,
                                  line_xyz=None, line_has=None):
        """Device-resident inputs and outputs (pack_local_lines' order, cur_kl .. Tcw): asynchronous on the handle's stream."""
        check(lib.msl_match_local_lines(self.h, n_frames, lcap, mlcap, ptr(params), *[ptr(a) for a in arrays], 1, ptr(match_out), ptr(n_to_match),
                                        ptr(nmatches), ptr(in_view), ptr(track), ptr(line_xyz), ptr(line_has), 1), "msl_match_local_lines")

    def descriptor_distance(self, a, b):
        a = np.ascontiguousarray(a, np.uint8).reshape(-1, 32); b = np.ascontiguousarray(b, np.uint8).reshape(-1, 32)
        out = np.zeros(len(a), np.int32)
        check(lib.msl_match_descriptor_distances(self.h, ptr(a), ptr(b), len(a), ptr(out)), "msl_match_descriptor_distances")
        return out


def search_by_projection_batch(params, cur, last, Tcw_cur, Tcw_last, device=0, handle=None):
    """cur / last: lists (one entry per pair) of dicts with the arrays msl.h names:
         cur:  kps (KEYPOINT_DTYPE), un_xy (N,2) f32, uright (N,) f32, grid_cell (N,) i32, desc (N,32) u8
         last: xyz (M,3) f32, desc (M,32) u8, flags (M,) u8, octave (M,) i32, angle (M,) f32
       Tcw_*: (n_pairs, 4, 4) or (n_pairs, 3, 4) float32, row-major.  Returns (match [n_pairs][N] i32 lists, nmatches)."""
    B = len(cur)
    cap = max(max(len(c["kps"]) for c in cur), max(len(l["xyz"]) for l in last), 1)
    arrays = _pack_cur(cur, cap) + [
        pad(last, "xyz", cap, np.float32, shape=(3,)), pad(last, "desc", cap, np.uint8, shape=(32,)), pad(last, "flags", cap, np.uint8),
        pad(last, "octave", cap, np.int32), pad(last, "angle", cap, np.float32), np.array([len(l["xyz"]) for l in last], np.int32),
        _rows3x4(Tcw_cur, B), _rows3x4(Tcw_last, B)]
    match = np.zeros((B, cap), np.int32); nm = np.zeros(B, np.int32)
    call("msl_match_by_projection", handle, device, B, cap, ptr(params), *[ptr(a) for a in arrays], MSL_MEM_HOST, ptr(match), ptr(nm),
         MSL_MEM_HOST)
    ncur = arrays[5]
    return [match[f, :ncur[f]].copy() for f in range(B)], nm


def _pack_cur(cur, cap):
    """cur_kps .. n_cur, the current-frame arrays both searches take."""
    return [pad(cur, "kps", cap, KEYPOINT_DTYPE), pad(cur, "un_xy", cap, np.float32, shape=(2,)), pad(cur, "uright", cap, np.float32),
            pad(cur, "grid_cell", cap, np.int32, -1), pad(cur, "desc", cap, np.uint8, shape=(32,)),
            np.array([len(c["kps"]) for c in cur], np.int32)]


def _rows3x4(Tcw, n_frames):
    """Rows 0-2 of each (4, 4) or (3, 4) mTcw, as the ABI's [frames][12] float32."""
    return np.ascontiguousarray(np.asarray(Tcw, np.float32)[:, :3, :4].reshape(n_frames, 12))


def descriptor_distance(a, b, device=0):
    a = np.ascontiguousarray(a, np.uint8).reshape(-1, 32); b = np.ascontiguousarray(b, np.uint8).reshape(-1, 32)
    out = np.zeros(len(a), np.int32)
    check(lib.msl_match_descriptor_distance(device, ptr(a), ptr(b), len(a), ptr(out)), "msl_match_descriptor_distance")
    return out


def pack_local_points(cur, local, Tcw, cap=None, mcap=None):
    """Packs per-frame dicts into msl_match_local_points' [frames][cap] / [frames][mcap] arrays (its argument order, cur_kps .. Tcw).
       cur:   kps (KEYPOINT_DTYPE), un_xy (N,2) f32, uright (N,) f32, grid_cell (N,) i32, desc (N,32) u8, flags (N,) u8
       local: xyz (M,3) f32, normal (M,3) f32, dist (M,2) f32 (mfMinDistance, mfMaxDistance), desc (M,32) u8, flags (M,) u8
       Tcw:   (n_frames, 4, 4) or (n_frames, 3, 4) float32, row-major."""
    cap = cap or max(max(len(c["kps"]) for c in cur), 1)
    mcap = mcap or max(max(len(l["xyz"]) for l in local), 1)
    return cap, mcap, _pack_cur(cur, cap) + [
        pad(cur, "flags", cap, np.uint8),
        pad(local, "xyz", mcap, np.float32, shape=(3,)), pad(local, "normal", mcap, np.float32, shape=(3,)),
        pad(local, "dist", mcap, np.float32, shape=(2,)), pad(local, "desc", mcap, np.uint8, shape=(32,)), pad(local, "flags", mcap, np.uint8),
        np.array([len(l["xyz"]) for l in local], np.int32), _rows3x4(Tcw, len(cur))]


def search_local_points_batch(params, cur, local, Tcw, device=0, handle=None, cap=None, mcap=None):
    """Tracking::SearchLocalPoints after its first loop, for a batch of frames (host arrays, synchronous); see pack_local_points for the
    inputs.  Returns (match: per frame (N,) i32 -- the local index written into mvpMapPoints[i2] or -1, n_to_match, nmatches,
    in_view: per frame (M,) u8, track: per frame (M,) LOCAL_TRACK_DTYPE)."""
    cap, mcap, arrays = pack_local_points(cur, local, Tcw, cap, mcap)
    B = len(cur)
    match = np.zeros((B, cap), np.int32); ntm = np.zeros(B, np.int32); nm = np.zeros(B, np.int32)
    inv = np.zeros((B, mcap), np.uint8); trk = np.zeros((B, mcap), LOCAL_TRACK_DTYPE)
    call("msl_match_local_points", handle, device, B, cap, mcap, ptr(params), *[ptr(a) for a in arrays], MSL_MEM_HOST, ptr(match), ptr(ntm), ptr(nm),
         ptr(inv), ptr(trk), MSL_MEM_HOST)
    ncur, nloc = arrays[5], arrays[12]
    return ([match[f, :ncur[f]].copy() for f in range(B)], ntm, nm, [inv[f, :nloc[f]].copy() for f in range(B)],
            [trk[f, :nloc[f]].copy() for f in range(B)])


def _pack_lines_cur(cur, lcap):
    """cur_kl, cur_ldesc, n_cur_lines: the current-frame arrays both line searches take."""
    return [pad(cur, "kl", lcap, KEYLINE_DTYPE), pad(cur, "desc", lcap, np.uint8, shape=(32,)), np.array([len(c["kl"]) for c in cur], np.int32)]


def _line_io(B, lcap, line_xyz, line_has):
    """The in/out pose-layout arrays: the caller's initial contents, or zeros."""
    lx = np.zeros((B, lcap, 6), np.float64) if line_xyz is None else np.array(line_xyz, np.float64).reshape(B, lcap, 6)
    lh = np.zeros((B, lcap), np.uint8) if line_has is None else np.array(line_has, np.uint8).reshape(B, lcap)
    return lx, lh


def pack_lines_last(cur, last, Tcw_cur, Tcw_last, lcap=None, llcap=None):
    """msl_match_lines_by_projection's inputs in its argument order (cur_kl .. Tcw_last).
       cur:  kl (N,) KEYLINE_DTYPE (mvKeylinesUn), desc (N,32) u8 (mLdesc)
       last: xyz (M,6) f64 (GetWorldPos), desc (M,32) u8, flags (M,) u8, octave (M,) i32"""
    B = len(cur)
    lcap = lcap or max(max(len(c["kl"]) for c in cur), 1)
    llcap = llcap or max(max(len(l["xyz"]) for l in last), 1)
    return lcap, llcap, _pack_lines_cur(cur, lcap) + [
        pad(last, "xyz", llcap, np.float64, shape=(6,)), pad(last, "desc", llcap, np.uint8, shape=(32,)), pad(last, "flags", llcap, np.uint8),
        pad(last, "octave", llcap, np.int32), np.array([len(l["xyz"]) for l in last], np.int32), _rows3x4(Tcw_cur, B), _rows3x4(Tcw_last, B)]


def search_lines_by_projection_batch(params, cur, last, Tcw_cur, Tcw_last, device=0, handle=None, lcap=None, llcap=None, line_xyz=None,
                                     line_has=None):
    """LSDmatcher::SearchByProjection(CurrentFrame, LastFrame, th) for a batch of frame pairs (host arrays, synchronous); see pack_lines_last.
    line_xyz / line_has: initial contents of the pose-layout outputs (default zeros).  Returns (match: per frame (N,) i32, nmatches,
    line_xyz [B][lcap][6] f64, line_has [B][lcap] u8)."""
    lcap, llcap, arrays = pack_lines_last(cur, last, Tcw_cur, Tcw_last, lcap, llcap)
    B = len(cur)
    match = np.zeros((B, lcap), np.int32); nm = np.zeros(B, np.int32)
    lx, lh = _line_io(B, lcap, line_xyz, line_has)
    call("msl_match_lines_by_projection", handle, device, B, lcap, llcap, ptr(params), *[ptr(a) for a in arrays], MSL_MEM_HOST, ptr(match), ptr(nm),
         ptr(lx), ptr(lh), MSL_MEM_HOST)
    ncur = arrays[2]
    return [match[f, :ncur[f]].copy() for f in range(B)], nm, lx, lh


def pack_local_lines(cur, local, Tcw, lcap=None, mlcap=None):
    """msl_match_local_lines' inputs in its argument order (cur_kl .. Tcw).
       cur:   kl (N,) KEYLINE_DTYPE, desc (N,32) u8, flags (N,) u8 (bit 0 held, bit 1 the holder has observations)
       local: xyz (M,6) f64, normal (M,3) f64, dist (M,2) f32 (mfMinDistance, mfMaxDistance), desc (M,32) u8, flags (M,) u8"""
    lcap = lcap or max(max(len(c["kl"]) for c in cur), 1)
    mlcap = mlcap or max(max(len(l["xyz"]) for l in local), 1)
    return lcap, mlcap, _pack_lines_cur(cur, lcap) + [
        pad(cur, "flags", lcap, np.uint8), pad(local, "xyz", mlcap, np.float64, shape=(6,)), pad(local, "normal", mlcap, np.float64, shape=(3,)),
        pad(local, "dist", mlcap, np.float32, shape=(2,)), pad(local, "desc", mlcap, np.uint8, shape=(32,)), pad(local, "flags", mlcap, np.uint8),
        np.array([len(l["xyz"]) for l in local], np.int32), _rows3x4(Tcw, len(cur))]


def search_local_lines_batch(params, cur, local, Tcw, device=0, handle=None, lcap=None, mlcap=None, line_xyz=None, line_has=None):
    """Tracking::SearchLocalLines after its first loop for a batch of frames (host arrays, synchronous); see pack_local_lines.  Returns
    (match: per frame (N,) i32, n_to_match, nmatches, in_view: per frame (M,) u8, track: per frame (M,) LINE_TRACK_DTYPE,
    line_xyz [B][lcap][6] f64, line_has [B][lcap] u8)."""
    lcap, mlcap, arrays = pack_local_lines(cur, local, Tcw, lcap, mlcap)
    B = len(cur)
    match = np.zeros((B, lcap), np.int32); ntm = np.zeros(B, np.int32); nm = np.zeros(B, np.int32)
    inv = np.zeros((B, mlcap), np.uint8); trk = np.zeros((B, mlcap), LINE_TRACK_DTYPE)
    lx, lh = _line_io(B, lcap, line_xyz, line_has)
    call("msl_match_local_lines", handle, device, B, lcap, mlcap, ptr(params), *[ptr(a) for a in arrays], MSL_MEM_HOST, ptr(match), ptr(ntm), ptr(nm),
         ptr(inv), ptr(trk), ptr(lx), ptr(lh), MSL_MEM_HOST)
    ncur, nloc = arrays[2], arrays[9]
    return ([match[f, :ncur[f]].copy() for f in range(B)], ntm, nm, [inv[f, :nloc[f]].copy() for f in range(B)],
            [trk[f, :nloc[f]].copy() for f in range(B)], lx, lh)

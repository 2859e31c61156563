"""Host mirror of ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th) (reference src/ORBmatcher.cc:547-678) through the
C ABI, for a batch of independent frame pairs, and of the local-map search Tracking::SearchLocalPoints
(src/Tracking.cc:1654-1695: isInFrustum + SearchByProjection(Frame&, vector<MapPoint*>, th)) for a batch of frames."""
import numpy as np

from ._lib import KEYPOINT_DTYPE, LOCAL_MATCH_PARAMS_DTYPE, LOCAL_TRACK_DTYPE, MATCH_PARAMS_DTYPE, MSL_MEM_HOST, call, check, lib, pad, ptr


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

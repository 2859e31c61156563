"""Host mirror of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:303-522) with ORBmatcher::SearchForTriangulation
(src/ORBmatcher.cc:257-406) through the C ABI: the new map points a batch of keyframes creates against their neighbours
(triangulate_new_points), the device-memory form (triangulate_new_points_device) and the per-pair stage of the last call (debug_triangulate)."""
import numpy as np

from ._lib import KEYPOINT_DTYPE, MSL_MEM_DEVICE, MSL_MEM_HOST, TRIANGULATE_PARAMS_DTYPE, call, check, fill_levels, lib, pad, ptr

# MSL_TRI_*: what became of a pair (idx1, match12)
(NO_MATCH, TRIANGULATED, STEREO1, STEREO2, NEIGHBOUR_SKIPPED, LOW_PARALLAX, W_ZERO, Z1, Z2, REPROJ1, REPROJ2, ZERO_DIST, SCALE) = range(13)
MAX_CAP, MAX_NCAP = 8192, 16
TABLE_KEYS = ("kps_un", "raw_xy", "uright", "depth", "desc", "node", "held", "n_kps", "Tcw")
OUT_KEYS = ("match12", "status", "nmatches", "new_neigh", "new_idx2", "new_xyz", "new_normal", "new_dist", "new_desc", "new_order", "n_new")


def triangulate_params(fx, fy, cx, cy, bf, scale_factors, level_sigma2, scale_factor, check_orientation=False, only_stereo=False, invfx=None,
                       invfy=None, b=None):
    """msl_triangulate_params.  invfx / invfy default to 1.0f / fx, 1.0f / fy and b to bf / fx in float, as the reference forms them; the call
    site's ORBmatcher(0.6, false) and bOnlyStereo = false are the defaults."""
    p = np.zeros(1, TRIANGULATE_PARAMS_DTYPE)
    f = np.float32
    p["fx"], p["fy"], p["cx"], p["cy"], p["bf"] = fx, fy, cx, cy, bf
    p["invfx"] = f(1.0) / f(fx) if invfx is None else invfx
    p["invfy"] = f(1.0) / f(fy) if invfy is None else invfy
    p["b"] = f(bf) / f(fx) if b is None else b
    fill_levels(p, scale_factors=scale_factors, level_sigma2=level_sigma2)
    p["scale_factor"], p["check_orientation"], p["only_stereo"] = scale_factor, int(check_orientation), int(only_stereo)
    return p


def pack_table(keyframes, cap=None):
    """Packs per-keyframe dicts into the keyframe table.  keyframe: kps_un (n,) KEYPOINT_DTYPE, raw_xy (n, 2) f32, uright, depth (n,) f32,
    desc (n, 32) u8, node (n,) i32, held (n,) u8, Tcw (3, 4) f32.  Returns (cap, dict of arrays named as in msl.h)."""
    cap = cap or max(max(len(k["kps_un"]) for k in keyframes), 1)
    return cap, dict(kps_un=pad(keyframes, "kps_un", cap, KEYPOINT_DTYPE), raw_xy=pad(keyframes, "raw_xy", cap, np.float32, shape=(2,)),
                     uright=pad(keyframes, "uright", cap, np.float32, fill=-1), depth=pad(keyframes, "depth", cap, np.float32, fill=-1),
                     desc=pad(keyframes, "desc", cap, np.uint8, shape=(32,)), node=pad(keyframes, "node", cap, np.int32, fill=-1),
                     held=pad(keyframes, "held", cap, np.uint8), n_kps=np.array([len(k["kps_un"]) for k in keyframes], np.int32),
                     Tcw=np.stack([np.asarray(k["Tcw"], np.float32).reshape(12) for k in keyframes]))


def pack_items(items, ncap=None):
    """items: [(cur, [neighbour table indices in covisibility order])] -> (ncap, cur, neigh [items][ncap] (-1 padded), n_neigh)."""
    ncap = ncap or max(max(len(nb) for _, nb in items), 1)
    cur = np.array([c for c, _ in items], np.int32)
    neigh = np.full((len(items), ncap), -1, np.int32)
    for f, (_, nb) in enumerate(items):
        neigh[f, :len(nb)] = nb
    return ncap, cur, neigh, np.array([len(nb) for _, nb in items], np.int32)


def outputs(n_items, ncap, cap, zeros=np.zeros):
    """The output arrays of one call, in msl.h's order (zeros(shape, dtype) allocates)."""
    F, R, C = n_items, ncap, cap
    return dict(match12=zeros((F, R, C), np.int32), status=zeros((F, R, C), np.uint8), nmatches=zeros((F, R), np.int32),
                new_neigh=zeros((F, C), np.int32), new_idx2=zeros((F, C), np.int32), new_xyz=zeros((F, C, 3), np.float32),
                new_normal=zeros((F, C, 3), np.float32), new_dist=zeros((F, C, 2), np.float32), new_desc=zeros((F, C, 32), np.uint8),
                new_order=zeros((F, C), np.int32), n_new=zeros((F,), np.int32))


def triangulate_new_points(params, keyframes, items, device=0, handle=None, cap=None, ncap=None):
    """msl_triangulate_new_points on host arrays (synchronous); see pack_table / pack_items.  Returns a dict of the outputs (OUT_KEYS)."""
    cap, t = pack_table(keyframes, cap)
    ncap, cur, neigh, n_neigh = pack_items(items, ncap)
    out = outputs(len(items), ncap, cap)
    call("msl_triangulate_new_points", handle, device, len(keyframes), cap, len(items), ncap, ptr(params), *[ptr(t[k]) for k in TABLE_KEYS], ptr(cur),
         ptr(neigh), ptr(n_neigh), MSL_MEM_HOST, *[ptr(out[k]) for k in OUT_KEYS], MSL_MEM_HOST)
    return out


def triangulate_new_points_device(handle, params, n_tab, cap, n_items, ncap, table, cur, neigh, n_neigh, out):
    """Device-resident inputs and outputs (torch tensors / device pointers: `table` keyed by TABLE_KEYS, `out` by OUT_KEYS) on a match.Matcher:
    asynchronous on the handle's stream."""
    check(lib.msl_triangulate_new_points(handle.h, n_tab, cap, n_items, ncap, ptr(params), *[ptr(table[k]) for k in TABLE_KEYS], ptr(cur), ptr(neigh),
                                         ptr(n_neigh), MSL_MEM_DEVICE, *[ptr(out[k]) for k in OUT_KEYS], MSL_MEM_DEVICE), "msl_triangulate_new_points")


def debug_triangulate(handle, item, neigh, cap):
    """One (item, neighbour) pair of the last call on a match.Matcher (cap: that call's): dict(F12 (3, 3), ex, ey, baseline, idx2 (cap,), bin
    (cap,), cos (cap, 3) = cosParallaxRays / Stereo1 / Stereo2, x3d (cap, 4)) -- the candidates before the rotation cull and the chain."""
    pair = np.zeros(12, np.float32); cand = np.zeros((cap, 2), np.int32); cos = np.zeros((cap, 3), np.float32); x3d = np.zeros((cap, 4), np.float32)
    check(lib.msl_debug_triangulate(handle.h, item, neigh, ptr(pair), ptr(cand), ptr(cos), ptr(x3d)), "msl_debug_triangulate")
    return dict(F12=pair[:9].reshape(3, 3).copy(), ex=pair[9], ey=pair[10], baseline=pair[11], idx2=cand[:, 0].copy(), bin=cand[:, 1].copy(), cos=cos,
                x3d=x3d)


__all__ = ["triangulate_params", "pack_table", "pack_items", "outputs", "triangulate_new_points", "triangulate_new_points_device",
           "debug_triangulate", "TABLE_KEYS", "OUT_KEYS"]

"""Host mirror of the plane clouds through the C ABI for a batch of independent frames: the tail of Frame::ExtractPlanes (reference
src/Frame.cc:611-653, :662-709; msl_plane_clouds[_batch]) and the map-plane merge of src/Tracking.cc:429-436 over
MapPlane::UpdateCoefficientsAndPoints (src/MapPlane.cc:201-218; msl_map_plane_merge[_batch]).  A frame is a dict of numpy arrays, named
as in tests/plane_cloud_model.py:
  msl_plane_clouds     cloud (V,3) f64 (msl_peac_extract_batch's cloud_out), rgb (V,3) u8 or None, vertices: one index array per detector
                       plane, planes: one (normal (3,), center (3,)) per detector plane, seed
  msl_map_plane_merge  clouds: one (n,3) f32 per frame plane, rgbs: the same in u8 or None, merge_into: a map row or -1 per frame plane,
                       Twc (12,) f64 (rows 0-2, row-major), mp_clouds: one (n,3) f32 per map plane, mp_rgbs or None"""
import numpy as np

from ._lib import MSL_MEM_HOST, PEAC_PLANE_DTYPE, PLANE_CLOUD_PARAMS_DTYPE, call, check, lib, ptr

__all__ = ["PLANE_CLOUD_PARAMS_DTYPE", "MAX_VOXELS", "MAX_VERTICES", "plane_cloud_params", "pack_clouds", "pack_csr", "pack_merge",
           "plane_clouds_batch", "plane_clouds_device", "map_plane_merge_batch", "map_plane_merge_device"]

MAX_VOXELS = 4096                # MSL_PLANE_CLOUD_MAX_VOXELS
MAX_VERTICES = 1 << 17           # MSL_PLANE_CLOUD_MAX_VERTICES


def plane_cloud_params(leaf=0.2, dis_th=0.05, max_iterations=50, probability=0.99):
    """msl_plane_cloud_params: the voxel leaf, Plane.DistanceThreshold, and SACSegmentation's max_iterations and probability."""
    p = np.zeros(1, PLANE_CLOUD_PARAMS_DTYPE)
    p["leaf"], p["dis_th"], p["max_iterations"], p["probability"] = leaf, dis_th, max_iterations, probability
    return p


def pack_clouds(frames, n_vertices=None, max_planes=None):
    """Packs per-frame dicts into msl_plane_clouds' inputs.  Returns (n_vertices, max_planes, has_rgb, inputs in ABI order cloud .. seed;
    rgb is None when no frame carries colour)."""
    F = len(frames)
    V = n_vertices or max(max(len(fr["cloud"]) for fr in frames), 1)
    P = max_planes or max(max(len(fr["planes"]) for fr in frames), 1)
    has_rgb = frames[0].get("rgb") is not None
    cloud = np.zeros((F, V, 3), np.float64)
    rgb = np.zeros((F, V, 3), np.uint8) if has_rgb else None
    off = np.zeros((F, P + 1), np.int32)
    idx = np.zeros((F, V), np.int32)
    planes = np.zeros((F, P), PEAC_PLANE_DTYPE)
    for f, fr in enumerate(frames):
        cloud[f, :len(fr["cloud"])] = fr["cloud"]
        if has_rgb:
            rgb[f, :len(fr["rgb"])] = fr["rgb"]
        o = 0
        for i, v in enumerate(fr["vertices"]):
            idx[f, o:o + len(v)] = v
            o += len(v)
            off[f, i + 1] = o
        off[f, len(fr["vertices"]) + 1:] = o
        for i, (normal, center) in enumerate(fr["planes"]):
            planes[f, i]["normal"], planes[f, i]["center"] = normal, center
    inputs = [cloud, rgb, off, idx, planes, np.array([len(fr["planes"]) for fr in frames], np.int32),
              np.array([int(fr["seed"]) & 0xFFFFFFFF for fr in frames], np.uint32)]
    return V, P, has_rgb, inputs


def pack_csr(clouds, rgbs, rows, cap=None):
    """Per-frame lists of clouds as CSR: (cap, off [frames][rows + 1] i32, pts [frames][cap][3] f32, rgb [frames][cap][3] u8 or None)."""
    F = len(clouds)
    cap = cap or max(max(sum(len(c) for c in cs) for cs in clouds), 1)
    off = np.zeros((F, rows + 1), np.int32)
    pts = np.zeros((F, cap, 3), np.float32)
    rgb = np.zeros((F, cap, 3), np.uint8) if rgbs is not None else None
    for f, cs in enumerate(clouds):
        o = 0
        for j, c in enumerate(cs):
            c = np.asarray(c, np.float32).reshape(-1, 3)
            pts[f, o:o + len(c)] = c
            if rgb is not None:
                rgb[f, o:o + len(c)] = np.asarray(rgbs[f][j], np.uint8).reshape(-1, 3)
            o += len(c)
            off[f, j + 1] = o
        off[f, len(cs) + 1:] = o
    return cap, off, pts, rgb


def pack_merge(frames, pcap=None, fptcap=None, mcap=None, ptcap=None):
    """Packs per-frame dicts into msl_map_plane_merge's inputs.  Returns (caps (pcap, fptcap, mcap, ptcap), inputs in ABI order n_planes ..
    n_map)."""
    pcap = pcap or max(max(len(fr["clouds"]) for fr in frames), 1)
    mcap = mcap or max(max(len(fr["mp_clouds"]) for fr in frames), 1)
    has_rgb = frames[0].get("mp_rgbs") is not None
    fptcap, off, pts, rgb = pack_csr([fr["clouds"] for fr in frames], [fr["rgbs"] for fr in frames] if has_rgb else None, pcap, fptcap)
    mptcap, moff, mpts, mrgb = pack_csr([fr["mp_clouds"] for fr in frames], [fr["mp_rgbs"] for fr in frames] if has_rgb else None, mcap, ptcap)
    into = np.full((len(frames), pcap), -1, np.int32)
    for f, fr in enumerate(frames):
        into[f, :len(fr["merge_into"])] = fr["merge_into"]
    inputs = [np.array([len(fr["clouds"]) for fr in frames], np.int32), off, pts, rgb, into,
              np.array([fr["Twc"] for fr in frames], np.float64).reshape(len(frames), 12), moff, mpts, mrgb,
              np.array([len(fr["mp_clouds"]) for fr in frames], np.int32)]
    return (pcap, fptcap, mcap, mptcap), inputs


def plane_clouds_batch(params, frames, pcap=None, ptcap=None, device=0, handle=None, n_vertices=None, max_planes=None):
    """The tail of ExtractPlanes for a batch of frames (host arrays, synchronous).  params: plane_cloud_params(...).  Returns per frame a dict
    n_out, plane_coef (n,4), plane_npts (n,), plane_src (n,), pt_off (n + 1,), pts (m,3), rgb (m,3) or None, status (detector planes,)."""
    V, P, has_rgb, arrays = pack_clouds(frames, n_vertices, max_planes)
    F = len(frames)
    pcap = pcap or P
    ptcap = ptcap or pcap * MAX_VOXELS
    n_out = np.zeros(F, np.int32)
    coef = np.zeros((F, pcap, 4), np.float32)
    npts = np.zeros((F, pcap), np.int32)
    src = np.zeros((F, pcap), np.int32)
    off = np.zeros((F, pcap + 1), np.int32)
    pts = np.zeros((F, ptcap, 3), np.float32)
    rgb = np.zeros((F, ptcap, 3), np.uint8) if has_rgb else None
    status = np.zeros((F, P), np.int32)
    call("msl_plane_clouds", handle, device, F, V, P, pcap, ptcap, ptr(params), *[ptr(a) for a in arrays], MSL_MEM_HOST, ptr(n_out), ptr(coef),
         ptr(npts), ptr(src), ptr(off), ptr(pts), ptr(rgb), ptr(status), MSL_MEM_HOST)
    res = []
    for f, fr in enumerate(frames):
        n = int(n_out[f])
        m = int(off[f, n])
        res.append(dict(n_out=n, plane_coef=coef[f, :n].copy(), plane_npts=npts[f, :n].copy(), plane_src=src[f, :n].copy(),
                        pt_off=off[f, :n + 1].copy(), pts=pts[f, :m].copy(), rgb=rgb[f, :m].copy() if has_rgb else None,
                        status=status[f, :len(fr["planes"])].copy()))
    return res


def plane_clouds_device(handle, params, n_frames, n_vertices, max_planes, pcap, ptcap, arrays, n_out, plane_coef, plane_npts, plane_src, pt_off,
                        pts, rgb_out, status):
    """The device form on a match.Matcher handle: arrays (cloud .. seed, pack_clouds' order; rgb may be None) and the outputs are torch
    tensors on the handle's device.  Asynchronous on the handle's stream."""
    check(lib.msl_plane_clouds(handle.h, n_frames, n_vertices, max_planes, pcap, ptcap, ptr(params), *[ptr(a) for a in arrays], 1, ptr(n_out),
                               ptr(plane_coef), ptr(plane_npts), ptr(plane_src), ptr(pt_off), ptr(pts), ptr(rgb_out), ptr(status), 1),
          "msl_plane_clouds")


def map_plane_merge_batch(params, frames, caps=None, device=0, handle=None):
    """The map-plane merge for a batch of frames (host arrays, synchronous).  Returns per frame a dict clouds (one (n,3) f32 per map plane),
    rgbs (or None), pt_off (n_map + 1,), status (n_map,)."""
    (pcap, fptcap, mcap, ptcap), arrays = pack_merge(frames, *(caps or ()))
    F = len(frames)
    has_rgb = arrays[3] is not None
    off = np.zeros((F, mcap + 1), np.int32)
    pts = np.zeros((F, ptcap, 3), np.float32)
    rgb = np.zeros((F, ptcap, 3), np.uint8) if has_rgb else None
    status = np.zeros((F, mcap), np.int32)
    call("msl_map_plane_merge", handle, device, F, pcap, fptcap, mcap, ptcap, ptr(params), *[ptr(a) for a in arrays], MSL_MEM_HOST, ptr(off),
         ptr(pts), ptr(rgb), ptr(status), MSL_MEM_HOST)
    res = []
    for f, fr in enumerate(frames):
        n = len(fr["mp_clouds"])
        o = off[f, :n + 1].copy()
        res.append(dict(clouds=[pts[f, o[j]:o[j + 1]].copy() for j in range(n)],
                        rgbs=[rgb[f, o[j]:o[j + 1]].copy() for j in range(n)] if has_rgb else None, pt_off=o, status=status[f, :n].copy()))
    return res


def map_plane_merge_device(handle, params, n_frames, caps, arrays, mp_pt_off_out, mp_pts_out, mp_rgb_out, merge_status):
    """The device form on a match.Matcher handle: arrays (n_planes .. n_map, pack_merge's order; the colour arrays may be None) and the
    outputs are torch tensors on the handle's device.  Asynchronous on the handle's stream."""
    pcap, fptcap, mcap, ptcap = caps
    check(lib.msl_map_plane_merge(handle.h, n_frames, pcap, fptcap, mcap, ptcap, ptr(params), *[ptr(a) for a in arrays], 1, ptr(mp_pt_off_out),
                                  ptr(mp_pts_out), ptr(mp_rgb_out), ptr(merge_status), 1), "msl_map_plane_merge")

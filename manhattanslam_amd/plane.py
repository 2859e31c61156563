"""Host mirror of PlaneMatcher::SearchMapByCoefficients (reference src/PlaneMatcher.cpp:31-106) and Tracking::DetectManhattan
(src/Tracking.cc:651-844) through the C ABI (msl_plane_associate[_batch], msl_manhattan_detect[_batch]) for a batch of independent frames.
A frame is a dict of numpy arrays -- the per-frame inputs of include/msl.h, named as in tests/plane_match_model.py:
  plane_coef (K,4) f32, Tcw (12,) f32 (rows 0-2 of mTcw), plane_match (K,3) i32 (in/out, -1 = NULL), plane_npts (K,) i32,
  mp_w (M,4) f32, mp_flags (M,) u8 (bit 0 = !isBad()), mp_clouds: M arrays (n,3) f32 (mvPlanePoints),
  full (E,7) i32 {a, b, c, kf, ia, ib, ic}, part (E,5) i32 {a, b, kf, ia, ib} (any order: pack sorts them),
  kf_Rwc (R,9) f32, kf_coef: R arrays (Q,4) f32, kf_npts: R arrays (Q,) i32."""
import numpy as np

from ._lib import MSL_MEM_HOST, PLANE_PARAMS_DTYPE, call, check, lib, pad, ptr

# The limits of the plane chain (csrc/msl_plane_tables.h; include/msl.h states them per entry): frames of a call, planes of a frame, map
# planes, cloud points, entries of the full / partial Manhattan table, keyframe rows.  kfplanes and keyframe take theirs from here.
MAX_FRAMES, MAX_PCAP, MAX_MCAP, MAX_PTCAP, MAX_FCAP, MAX_QCAP, MAX_KCAP = 65535, 64, 4096, 1 << 22, 65536, 65536, 4096
# A Manhattan table entry: w keys (map-plane rows, ascending), the keyframe slot, the keyframe-plane index of every key
FULL_W, PART_W = 3, 2
FULL_STRIDE, PART_STRIDE = 2 * FULL_W + 1, 2 * PART_W + 1


def plane_params(d_th, a_th, ver_th, par_th, mf_ver_th=0.0):
    """msl_plane_params: Plane.AssociationDisRef, AssociationAngRef, VerticalThreshold, ParallelThreshold, MFVerticalThreshold."""
    p = np.zeros(1, PLANE_PARAMS_DTYPE)
    for k, v in zip(PLANE_PARAMS_DTYPE.names, (d_th, a_th, ver_th, par_th, mf_ver_th)):
        p[k] = v
    return p


def pack_clouds(frames, mcap, ptcap=None):
    """The map-plane clouds as CSR: (ptcap, mp_pt_off [frames][mcap + 1] i32, mp_pts [frames][ptcap][3] f32)."""
    F = len(frames)
    totals = [sum(len(c) for c in fr["mp_clouds"]) for fr in frames]
    ptcap = ptcap or max(max(totals), 1)
    off = np.zeros((F, mcap + 1), np.int32)
    pts = np.zeros((F, ptcap, 3), np.float32)
    for f, fr in enumerate(frames):
        o = 0
        for j, c in enumerate(fr["mp_clouds"]):
            c = np.asarray(c, np.float32).reshape(-1, 3)
            pts[f, o:o + len(c)] = c
            o += len(c)
            off[f, j + 1] = o
        off[f, len(fr["mp_clouds"]) + 1:] = o
    return ptcap, off, pts


def pack_associate(frames, pcap=None, mcap=None, ptcap=None):
    """Packs per-frame dicts into msl_plane_associate's arrays.  Returns (caps (pcap, mcap, ptcap), inputs in ABI order plane_coef ..
    n_map, plane_match [frames][pcap][3] i32 (in/out))."""
    pcap = pcap or max(max(len(f["plane_coef"]) for f in frames), 1)
    mcap = mcap or max(max(len(f["mp_w"]) for f in frames), 1)
    ptcap, off, pts = pack_clouds(frames, mcap, ptcap)
    count = lambda key: np.array([len(fr[key]) for fr in frames], np.int32)
    inputs = [pad(frames, "plane_coef", pcap, np.float32, shape=(4,)), count("plane_coef"), np.array([fr["Tcw"] for fr in frames], np.float32),
              pad(frames, "mp_w", mcap, np.float32, shape=(4,)), pad(frames, "mp_flags", mcap, np.uint8), off, pts, count("mp_w")]
    return (pcap, mcap, ptcap), inputs, pad(frames, "plane_match", pcap, np.int32, -1, shape=(3,))


def sort_full(full):
    """Full Manhattan entries {a, b, c, kf, ia, ib, ic} with each key sorted ascending (its keyframe indices along) and the table sorted
    by key: Map compares the keys as unordered sets (src/Map.cc:71-123)."""
    full = np.asarray(full, np.int32).reshape(-1, FULL_STRIDE)
    out = np.empty_like(full)
    for e, (a, b, c, kf, ia, ib, ic) in enumerate(full):
        pairs = sorted([(a, ia), (b, ib), (c, ic)], key=lambda x: x[0])
        out[e] = [pairs[0][0], pairs[1][0], pairs[2][0], kf, pairs[0][1], pairs[1][1], pairs[2][1]]
    return out[np.lexsort((out[:, 2], out[:, 1], out[:, 0]))] if len(out) else out


def sort_part(part):
    """Partial entries {a, b, kf, ia, ib}, normalised as sort_full does."""
    part = np.asarray(part, np.int32).reshape(-1, PART_STRIDE)
    out = part.copy()
    sw = out[:, 0] > out[:, 1]
    out[sw] = out[sw][:, [1, 0, 2, 4, 3]]
    return out[np.lexsort((out[:, 1], out[:, 0]))] if len(out) else out


def pack_manhattan(frames, pcap=None, mcap=None, fcap=None, qcap=None, kcap=None, plane_match=None):
    """Packs per-frame dicts into msl_manhattan_detect's arrays (tables sorted).  plane_match: the [frames][pcap][3] array to read (default:
    the frames' own).  Returns (caps (pcap, mcap, fcap, qcap, kcap), inputs in ABI order plane_coef .. kf_npts)."""
    F = len(frames)
    pcap = pcap or max(max(len(f["plane_coef"]) for f in frames), max(max((len(c) for c in f["kf_coef"]), default=0) for f in frames), 1)
    mcap = mcap or max(max(len(f["mp_w"]) for f in frames), 1)
    fulls = [sort_full(fr["full"]) for fr in frames]
    parts = [sort_part(fr["part"]) for fr in frames]
    fcap = fcap or max(max(len(x) for x in fulls), 1)
    qcap = qcap or max(max(len(x) for x in parts), 1)
    kcap = kcap or max(max(len(fr["kf_Rwc"]) for fr in frames), 1)
    ft = np.zeros((F, fcap, FULL_STRIDE), np.int32)
    pt = np.zeros((F, qcap, PART_STRIDE), np.int32)
    kR = np.zeros((F, kcap, 9), np.float32)
    kc = np.zeros((F, kcap, pcap, 4), np.float32)
    kn = np.zeros((F, kcap, pcap), np.int32)
    for f, fr in enumerate(frames):
        ft[f, :len(fulls[f])] = fulls[f]
        pt[f, :len(parts[f])] = parts[f]
        kR[f, :len(fr["kf_Rwc"])] = np.asarray(fr["kf_Rwc"], np.float32).reshape(-1, 9)
        for r, (c, n) in enumerate(zip(fr["kf_coef"], fr["kf_npts"])):
            kc[f, r, :len(c)] = c
            kn[f, r, :len(n)] = n
    if plane_match is None:
        plane_match = pad(frames, "plane_match", pcap, np.int32, -1, shape=(3,))
    count = lambda xs: np.array([len(x) for x in xs], np.int32)
    inputs = [pad(frames, "plane_coef", pcap, np.float32, shape=(4,)), pad(frames, "plane_npts", pcap, np.int32),
              np.array([len(fr["plane_coef"]) for fr in frames], np.int32), plane_match, pad(frames, "mp_flags", mcap, np.uint8),
              np.array([len(fr["mp_w"]) for fr in frames], np.int32), ft, count(fulls), pt, count(parts), kR, kc, kn]
    return (pcap, mcap, fcap, qcap, kcap), inputs


def plane_association_batch(params, frames, device=0, handle=None, caps=None):
    """SearchMapByCoefficients for a batch of frames (host arrays, synchronous).  params: plane_params(...).  Returns per frame a dict
    nmatches, plane_match (K,3), plane_w (K,12), plane_has (K,), pM (K,4)."""
    (pcap, mcap, ptcap), arrays, match = pack_associate(frames, *(caps or ()))
    F = len(frames)
    nm = np.zeros(F, np.int32)
    pw = np.zeros((F, pcap, 12), np.float32)
    ph = np.zeros((F, pcap), np.uint8)
    pM = np.zeros((F, pcap, 4), np.float32)
    call("msl_plane_associate", handle, device, F, pcap, mcap, ptcap, ptr(params), *[ptr(a) for a in arrays], MSL_MEM_HOST, ptr(match),
         ptr(nm), ptr(pw), ptr(ph), ptr(pM), MSL_MEM_HOST)
    res = []
    for f, fr in enumerate(frames):
        k = len(fr["plane_coef"])
        res.append(dict(nmatches=int(nm[f]), plane_match=match[f, :k].copy(), plane_w=pw[f, :k].copy(), plane_has=ph[f, :k].copy(),
                        pM=pM[f, :k].copy()))
    return res


def plane_association_device(handle, params, n_frames, caps, arrays, plane_match, nmatches, plane_w, plane_has, pM=None):
    """The device form on a match.Matcher handle: arrays (plane_coef .. n_map, pack_associate's order), plane_match (updated in place),
    nmatches, plane_w, plane_has and the optional pM are torch tensors on the handle's device.  Asynchronous on the handle's stream."""
    pcap, mcap, ptcap = caps
    check(lib.msl_plane_associate(handle.h, n_frames, pcap, mcap, ptcap, ptr(params), *[ptr(a) for a in arrays], 1, ptr(plane_match),
                                  ptr(nmatches), ptr(plane_w), ptr(plane_has), ptr(pM), 1), "msl_plane_associate")


def manhattan_detect_batch(params, frames, rcw=None, device=0, handle=None, caps=None, plane_match=None):
    """DetectManhattan for a batch of frames (host arrays, synchronous).  rcw: the frames' manhattanRcw before the call, (n_frames, 9)
    float32 (default zeros); it is replaced only where a frame finds a Manhattan frame.  Returns per frame
    (found, full, Rcw (9,) f32, choice (6,) i32)."""
    (pcap, mcap, fcap, qcap, kcap), arrays = pack_manhattan(frames, *(caps or ()), plane_match=plane_match)
    F = len(frames)
    R = np.zeros((F, 9), np.float32) if rcw is None else np.array(rcw, np.float32).reshape(F, 9)
    found = np.zeros(F, np.int32)
    full = np.zeros(F, np.int32)
    choice = np.zeros((F, 6), np.int32)
    call("msl_manhattan_detect", handle, device, F, pcap, mcap, fcap, qcap, kcap, ptr(params), *[ptr(a) for a in arrays], MSL_MEM_HOST,
         ptr(found), ptr(full), ptr(R), ptr(choice), MSL_MEM_HOST)
    return [(int(found[f]), int(full[f]), R[f].copy(), choice[f].copy()) for f in range(F)]


def manhattan_detect_device(handle, params, n_frames, caps, arrays, found, full, rcw, choice=None):
    """The device form on a match.Matcher handle: arrays (pack_manhattan's order; tables sorted), found, full, rcw (in/out) and the optional
    choice are torch tensors on the handle's device.  Asynchronous on the handle's stream."""
    pcap, mcap, fcap, qcap, kcap = caps
    check(lib.msl_manhattan_detect(handle.h, n_frames, pcap, mcap, fcap, qcap, kcap, ptr(params), *[ptr(a) for a in arrays], 1,
                                   ptr(found), ptr(full), ptr(rcw), ptr(choice), 1), "msl_manhattan_detect")

"""Fixed scenes for msl_points_3d and msl_keyframe_decision (tests/keyframe_model.py is their model): random frames whose depths include
ties, the threshold itself, zeros, negatives, NaN and inf and whose slots mix NULL, held and held-without-observations; the ragged batch, the
full-capacity frames, and the frames of the keyframe decision.  Everything is seeded; model results are computed once and shared."""
import functools

import numpy as np

from tests import keyframe_model as km

F32 = np.float32
N_PTS, N_LINES, N_TAB = 600, 90, 5
RAGGED = (0, 1, 99, 100, 101, 102, 127, 128, 129, 257, 1000, 4097)     # the stop boundary, the wave boundary, a sort that is no power of two
FULL = (8192, 8191, 8192)                                              # every slot a member; one fewer; all depths equal
FILL = 0x5A


def keypoint_dtype():
    return np.dtype({"names": ["x", "y", "size", "angle", "response", "octave", "class_id"], "formats": ["<f4"] * 5 + ["<i4"] * 2, "itemsize": 28})


def pose(rng):
    """rows 0-2 of a rigid Tcw."""
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    q *= np.sign(np.linalg.det(q))
    return np.concatenate([q, rng.uniform(-2, 2, (3, 1))], 1).astype(F32)


def table(seed=5):
    """The map's side: pt_nobs (a third without observations), pt_flags, ln_nobs, and N_TAB keyframe rows of held ids."""
    rng = np.random.default_rng(seed)
    pt_nobs = rng.integers(0, 6, N_PTS).astype(np.int32)
    pt_nobs[rng.random(N_PTS) < 0.3] = 0
    pt_flags = (rng.random(N_PTS) < 0.85).astype(np.uint8)
    ln_nobs = rng.integers(0, 4, N_LINES).astype(np.int32)
    rows = [np.where(rng.random(n) < 0.7, rng.integers(0, N_PTS, n), -1).astype(np.int32) for n in (0, 1, 64, 257, 300)]
    return dict(pt_nobs=pt_nobs, pt_flags=pt_flags, ln_nobs=ln_nobs, rows=rows)


def point_frame(seed, n, th_depth=3.0, members=None, equal=False, held=0.5, bad_octave=0.02):
    """One frame of n slots.  members: None = depths of every kind, "all" = every depth positive."""
    rng = np.random.default_rng(1000 + seed)
    kps = np.zeros(n, keypoint_dtype())
    kps["x"], kps["y"] = rng.uniform(0, 640, n).astype(F32), rng.uniform(0, 480, n).astype(F32)
    kps["octave"] = rng.integers(0, 8, n)
    odd = rng.random(n) < bad_octave                                    # octaves outside the levels
    kps["octave"][odd] = np.resize([8, -1, 99], int(odd.sum()))
    depth = (rng.integers(3, 61, n) * 0.1).astype(F32)                  # a grid of 58 values around th_depth: ties, and th_depth itself
    fine = rng.random(n) < 0.5
    depth[fine] = rng.uniform(0.3, 6.0, int(fine.sum())).astype(F32)
    if members is None:
        kind = rng.random(n)
        depth[kind < 0.05] = 0.0
        depth[(kind >= 0.05) & (kind < 0.10)] = -1.0
        depth[(kind >= 0.10) & (kind < 0.12)] = np.nan
        depth[(kind >= 0.12) & (kind < 0.14)] = np.inf
        depth[(kind >= 0.14) & (kind < 0.17)] = F32(th_depth)
    if equal:
        depth[:] = F32(1.75)
    cur = np.full(n, -1, np.int32)
    h = rng.random(n) < held
    cur[h] = rng.integers(0, N_PTS, int(h.sum()))
    return dict(kps_un=kps, depth=depth, desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), Tcw=pose(rng), cur_held=cur)


@functools.lru_cache(maxsize=None)
def ragged():
    return tuple(point_frame(f, n) for f, n in enumerate(RAGGED))


@functools.lru_cache(maxsize=None)
def full():
    return (point_frame(50, FULL[0], members="all", held=0.8), point_frame(51, FULL[1], members="all", held=0.8),
            point_frame(52, FULL[2], members="all", equal=True, held=0.8))


def point_params(**kw):
    return km.params(**kw)


@functools.lru_cache(maxsize=None)
def point_model(which, mode, cap, first=False, enable=None):
    """The model's outputs for the frames of `which` ("ragged" / "full"), stacked as the ABI lays them out: [frames][cap, ...]."""
    frames = ragged() if which == "ragged" else full()
    t = table()
    res = [km.points_3d(mode, point_params(), fr["kps_un"], fr["depth"], fr["desc"], fr["Tcw"], fr["cur_held"], t["pt_nobs"],
                        enable=True if enable is None else bool(enable[f]), first_id=1000 * f + 7 if first else None, cap=cap)
           for f, fr in enumerate(frames)]
    return stack(res)


def stack(res):
    out = {k: np.stack([np.asarray(r[k]) for r in res]) for k in res[0]}
    out["n_new"], out["n_walked"] = out["n_new"].astype(np.int32), out["n_walked"].astype(np.int32)
    return out


# ---- the keyframe decision ------------------------------------------------------------------------------------------------------------------
RECORD = dict(flags=km.TRACKED_LOCAL_MAP, frame_id=100, last_keyframe_id=95, last_reloc_frame_id=0, n_kfs=10, ref_kf=3, n_inliers_in=0,
              local_mapping_idle=1, local_mapping_stopped=0, keyframes_in_queue=0)
DECISION_PARAMS = dict(max_frames=30, min_frames=0, th_depth=F32(3.0), only_tracking=0)


def decision_frame(seed, n, nl, npl, **record):
    rng = np.random.default_rng(2000 + seed)
    p = point_frame(seed, n, held=0.7)
    lheld = np.where(rng.random(nl) < 0.7, rng.integers(0, N_LINES, nl), -1).astype(np.int32)
    return dict(RECORD, depth=p["depth"], cur_held=p["cur_held"], outlier=(rng.random(n) < 0.2).astype(np.uint8), cur_lheld=lheld,
                line_outlier=(rng.random(nl) < 0.3).astype(np.uint8),
                plane_match=np.where(rng.random((npl, 3)) < 0.6, rng.integers(0, 9, (npl, 3)), -1).astype(np.int32),
                plane_outlier=(rng.random((npl, 3)) < 0.4).astype(np.uint8), **record)


@functools.lru_cache(maxsize=None)
def decision_frames():
    """One ragged batch: lines 1, 40, 256 and planes 0, 1, pcap = 64 among them; every early return, both idle branches, a skipped step 1."""
    T, O, P = km.TRACKED_LOCAL_MAP, km.TRACK_OK, km.NEW_PLANE
    return (decision_frame(0, 1000, 40, 3), decision_frame(1, 0, 1, 0), decision_frame(2, 1, 1, 1), decision_frame(3, 257, 256, 64),
            decision_frame(4, 129, 40, 2, flags=O, n_inliers_in=40), decision_frame(5, 128, 7, 2, flags=O | P, n_inliers_in=400),
            decision_frame(6, 300, 9, 1, flags=0, n_inliers_in=99), decision_frame(7, 500, 3, 0, local_mapping_stopped=1),
            decision_frame(8, 64, 2, 5, last_reloc_frame_id=90, n_kfs=31), decision_frame(9, 63, 2, 5, last_reloc_frame_id=90, n_kfs=5),
            decision_frame(10, 700, 30, 4, local_mapping_idle=0, keyframes_in_queue=3, last_keyframe_id=10),
            decision_frame(11, 700, 30, 4, local_mapping_idle=0, keyframes_in_queue=2, last_keyframe_id=10),
            decision_frame(12, 4097, 1, 1, n_kfs=1, ref_kf=4), decision_frame(13, 90, 5, 2, ref_kf=-1, frame_id=-3, last_keyframe_id=-20),
            decision_frame(14, 15, 3, 2, last_reloc_frame_id=95))


@functools.lru_cache(maxsize=None)
def decision_model(only_tracking=0):
    t = table()
    prm = dict(DECISION_PARAMS, only_tracking=only_tracking)
    return tuple(km.keyframe_decision(prm, fr, t["rows"], t["pt_nobs"], t["pt_flags"], t["ln_nobs"]) for fr in decision_frames())


def table_arrays(cap):
    """held_id [N_TAB][cap] / n_kps of the keyframe table."""
    t = table()
    held = np.full((N_TAB, cap), -1, np.int32)
    for k, r in enumerate(t["rows"]):
        held[k, :min(len(r), cap)] = r[:cap]
    return held, np.array([min(len(r), cap) for r in t["rows"]], np.int32)


def decision_expected(cap, lcap, pcap, only_tracking=0):
    """The model's outputs as the ABI lays them out; plane_match / plane_outlier as they are left."""
    frames, res = decision_frames(), decision_model(only_tracking)
    F = len(frames)
    e = dict(found_pt=np.zeros((F, cap), np.uint8), found_line=np.zeros((F, lcap), np.uint8), n_inliers=np.zeros(F, np.int32), track_ok=np.zeros(F, np.uint8),
             new_plane=np.zeros(F, np.uint8), held_out=np.full((F, cap), -1, np.int32), outlier_out=np.zeros((F, cap), np.uint8),
             lheld_out=np.full((F, lcap), -1, np.int32), line_outlier_out=np.zeros((F, lcap), np.uint8), counts=np.zeros((F, 4), np.int32),
             cond=np.zeros(F, np.uint8), need_kf=np.zeros(F, np.int32), plane_match=np.full((F, pcap, 3), -1, np.int32),
             plane_outlier=np.zeros((F, pcap, 3), np.uint8))
    for f, r in enumerate(res):
        for k in ("found_pt", "held_out", "outlier_out", "found_line", "lheld_out", "line_outlier_out", "plane_match", "plane_outlier"):
            e[k][f, :len(r[k])] = r[k]
        for k in ("n_inliers", "track_ok", "new_plane", "counts", "cond", "need_kf"):
            e[k][f] = r[k]
    return e


def host_filled(shape, dtype):
    return np.frombuffer(bytes([FILL]) * (int(np.prod(shape)) * np.dtype(dtype).itemsize), dtype).reshape(shape).copy()

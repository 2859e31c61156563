"""Host mirror of the two relocalisation steps of Tracking::Relocalization (reference src/Tracking.cc:1909-2055) through the C ABI:
the keyframe database and KeyFrameDatabase::DetectRelocalizationCandidates (src/KeyFrameDatabase.cc:38-170: KeyFrameDatabase,
reloc_candidates), and ORBmatcher::SearchByProjection(Frame&, KeyFrame*, const set<MapPoint*>&, th, ORBdist) (src/ORBmatcher.cc:680-797)
for a batch of independent (frame, keyframe) pairs (search_keyframe_points)."""
import numpy as np

from ._lib import KEYFRAME_MATCH_PARAMS_DTYPE, MATCH_PARAMS_DTYPE, MSL_MEM_DEVICE, MSL_MEM_HOST, MslError, check, call, lib, pad, ptr
from .match import _pack_cur, _rows3x4, match_params


def keyframe_match_params(frame_params, scale_factors, th, orb_dist, log_scale_factor, check_orientation=True):
    """msl_keyframe_match_params: match_params(...) plus Frame::mfLogScaleFactor and ORBdist (Relocalization: th 10 / 100, then 3 / 64,
    for an ORBmatcher(0.9, true))."""
    p = np.zeros(1, KEYFRAME_MATCH_PARAMS_DTYPE)
    b = match_params(frame_params, scale_factors, th, check_orientation)
    for k in MATCH_PARAMS_DTYPE.names:
        p[k] = b[k]
    p["log_scale_factor"], p["orb_dist"] = log_scale_factor, orb_dist
    return p


def pack_keyframe_points(cur, kf, Tcw, cap=None, kcap=None):
    """Packs per-pair dicts into msl_match_keyframe_points' [pairs][cap] / [pairs][kcap] arrays (its argument order, cur_kps .. Tcw).
       cur: kps (KEYPOINT_DTYPE), un_xy (N,2) f32, grid_cell (N,) i32, desc (N,32) u8, held (N,) u8
       kf:  xyz (M,3) f32, dist (M,2) f32 (mfMinDistance, mfMaxDistance), desc (M,32) u8, angle (M,) f32, flags (M,) u8
       Tcw: (n_pairs, 4, 4) or (n_pairs, 3, 4) float32, row-major."""
    cap = cap or max(max(len(c["kps"]) for c in cur), 1)
    kcap = kcap or max(max(len(k["xyz"]) for k in kf), 1)
    kps, un, _, cell, desc, ncur = _pack_cur([dict(c, uright=np.zeros(len(c["kps"]), np.float32)) for c in cur], cap)
    return cap, kcap, [kps, un, cell, desc, ncur, pad(cur, "held", cap, np.uint8),
                       pad(kf, "xyz", kcap, np.float32, shape=(3,)), pad(kf, "dist", kcap, np.float32, shape=(2,)),
                       pad(kf, "desc", kcap, np.uint8, shape=(32,)), pad(kf, "angle", kcap, np.float32), pad(kf, "flags", kcap, np.uint8),
                       np.array([len(k["xyz"]) for k in kf], np.int32), _rows3x4(Tcw, len(cur))]


def search_keyframe_points(params, cur, kf, Tcw, device=0, handle=None, cap=None, kcap=None):
    """SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) for every pair (host arrays, synchronous); see pack_keyframe_points.
    Returns (match: per pair (N,) i32 -- the keyframe keypoint index written into mvpMapPoints[i2] or -1, nmatches)."""
    cap, kcap, arrays = pack_keyframe_points(cur, kf, Tcw, cap, kcap)
    B = len(cur)
    match = np.zeros((B, cap), np.int32); nm = np.zeros(B, np.int32)
    call("msl_match_keyframe_points", handle, device, B, cap, kcap, ptr(params), *[ptr(a) for a in arrays], MSL_MEM_HOST, ptr(match), ptr(nm),
         MSL_MEM_HOST)
    ncur = arrays[4]
    return [match[f, :ncur[f]].copy() for f in range(B)], nm


def search_keyframe_points_device(handle, params, n_pairs, cap, kcap, arrays, match_out, nmatches):
    """Device-resident inputs and outputs (torch tensors / device pointers in msl.h's argument order, cur_kps .. Tcw) on a
    match.Matcher: asynchronous on the handle's stream."""
    check(lib.msl_match_keyframe_points(handle.h, n_pairs, cap, kcap, ptr(params), *[ptr(a) for a in arrays], 1, ptr(match_out), ptr(nmatches), 1),
          "msl_match_keyframe_points")


class KeyFrameDatabase:
    """One msl_kfdb: the BowVectors of the keyframes on one device, one slot per add (never reused before clear)."""

    def __init__(self, device=0):
        self.h = lib.msl_kfdb_create(device)
        if not self.h:
            raise MslError(lib.msl_last_error().decode())
        self.device = device

    def add(self, bow_word, bow_value, n_words=None, handle=None):
        """KeyFrameDatabase::add.  Host arrays (n_words defaults to their length), or device tensors as msl_bow_transform wrote them with
        n_words a device int32 and handle the Matcher that produced them (the call waits for its stream).  Returns the slot."""
        slot = np.zeros(1, np.int32)
        if hasattr(bow_word, "data_ptr"):
            check(lib.msl_kfdb_add(self.h, handle.h, ptr(bow_word), ptr(bow_value), ptr(n_words), MSL_MEM_DEVICE, ptr(slot)), "msl_kfdb_add")
        else:
            w = np.ascontiguousarray(bow_word, np.int32); v = np.ascontiguousarray(bow_value, np.float64)
            n = np.array([len(w) if n_words is None else n_words], np.int32)
            w = w if len(w) else np.zeros(1, np.int32); v = v if len(v) else np.zeros(1, np.float64)
            check(lib.msl_kfdb_add(self.h, handle.h if handle is not None else None, ptr(w), ptr(v), ptr(n), MSL_MEM_HOST, ptr(slot)), "msl_kfdb_add")
        return int(slot[0])

    def erase(self, slot):
        check(lib.msl_kfdb_erase(self.h, int(slot)), "msl_kfdb_erase")

    def clear(self):
        check(lib.msl_kfdb_clear(self.h), "msl_kfdb_clear")

    def size(self):
        """(slots handed out since the last clear, live keyframes)"""
        a = np.zeros(1, np.int32); b = np.zeros(1, np.int32)
        check(lib.msl_kfdb_size(self.h, ptr(a), ptr(b)), "msl_kfdb_size")
        return int(a[0]), int(b[0])

    def close(self):
        if getattr(self, "h", None):
            lib.msl_kfdb_destroy(self.h)
            self.h = None

    __del__ = close


def pack_covis(covis, n_slots):
    """covis: per slot the list of covisible slots (at most 10, in order) -> the ABI's [n_slots][10] int32, -1 terminated."""
    out = np.full((max(n_slots, 1), 10), -1, np.int32)
    for s, row in enumerate(covis[:n_slots]):
        out[s, :len(row)] = row
    return out


def reloc_candidates(db, vocab, frames, covis, ccap=None, cap=None, handle=None, device=0, details=True):
    """DetectRelocalizationCandidates for consecutive query frames (dicts with bow_word (W,) i32 ascending and bow_value (W,) f64, as
    bow.transform returns them).  covis: see pack_covis.  Returns (candidates: per frame the slots in the reference's order, cut at ccap;
    n_cand: the full counts; words [F][n_slots] i32 and scores [F][n_slots] f32, or None without details)."""
    F = len(frames)
    n_slots = db.size()[0]
    cap = cap or max(max(len(f["bow_word"]) for f in frames), 1)
    ccap = ccap or max(n_slots, 1)
    bw = pad(frames, "bow_word", cap, np.int32); bv = pad(frames, "bow_value", cap, np.float64)
    nw = np.array([len(f["bow_word"]) for f in frames], np.int32)
    cv = pack_covis(covis, n_slots)
    cand = np.full((F, ccap), -1, np.int32); nc = np.zeros(F, np.int32)
    words = np.zeros((F, max(n_slots, 1)), np.int32) if details else None
    score = np.zeros((F, max(n_slots, 1)), np.float32) if details else None
    args = (db.h, vocab.h, F, cap, ccap, ptr(bw), ptr(bv), ptr(nw), ptr(cv), MSL_MEM_HOST, ptr(cand), ptr(nc), ptr(words), ptr(score), MSL_MEM_HOST)
    call("msl_reloc_candidates", handle, device, *args)
    res = [cand[f, :min(nc[f], ccap)].copy() for f in range(F)], nc
    return res + ((words[:, :n_slots], score[:, :n_slots]) if details else (None, None))


def reloc_candidates_device(handle, db, vocab, n_frames, cap, ccap, bow_word, bow_value, n_words, covis, cand_out, n_cand, words_out=None,
                            score_out=None):
    """Device-resident inputs and outputs (torch tensors / device pointers as msl_bow_transform wrote them; covis [n_slots][10] int32,
    words_out / score_out [n_frames][n_slots] or None) on a match.Matcher: asynchronous on the handle's stream."""
    check(lib.msl_reloc_candidates(handle.h, db.h, vocab.h, n_frames, cap, ccap, ptr(bow_word), ptr(bow_value), ptr(n_words), ptr(covis),
                                   MSL_MEM_DEVICE, ptr(cand_out), ptr(n_cand), ptr(words_out), ptr(score_out), MSL_MEM_DEVICE), "msl_reloc_candidates")


__all__ = ["KeyFrameDatabase", "pack_covis", "reloc_candidates", "reloc_candidates_device", "keyframe_match_params", "pack_keyframe_points", "search_keyframe_points", "search_keyframe_points_device"]

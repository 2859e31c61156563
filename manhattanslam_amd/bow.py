"""Host mirror of the bag-of-words layer through the C ABI: the device vocabulary (DBoW2::TemplatedVocabulary, reference
Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h), Frame::ComputeBoW / KeyFrame::ComputeBoW (msl_bow_transform[_batch]),
ORBmatcher::SearchByBoW(KeyFrame*, Frame&) (src/ORBmatcher.cc:146-247, msl_match_by_bow[_batch]) and LSDmatcher::SearchByDescriptor
(src/LSDmatcher.cpp:201-234, msl_match_lines_by_descriptor[_batch]), for batches of independent frames / pairs.
Frames and pairs are dicts of numpy arrays, named as in tests/bow_model.py:
  transform   desc (N,32) u8
  SearchByBoW kf_desc (N,32) u8, kf_angle (N,) f32, kf_node (N,) i32, kf_flags (N,) u8 (bit 0 = map point held and not bad),
              cur_angle (M,) f32 (mvKeys[i].angle), cur_desc (M,32) u8, cur_node (M,) i32
  lines       kf_ldesc (Q,32) u8, kf_flags (Q,) u8 (bit 0 = map line held), optional kf_xyz (Q,6) f64, cur_ldesc (T,32) u8"""
import numpy as np

from ._lib import BOW_MATCH_PARAMS_DTYPE, KEYPOINT_DTYPE, MSL_MEM_HOST, MslError, call, check, lib, pad, ptr

TF_IDF, TF, IDF, BINARY = range(4)                                             # DBoW2::WeightingType
L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT = range(6)       # DBoW2::ScoringType


class Vocabulary:
    """One msl_vocab: the node table of a DBoW2 vocabulary on one device.  Arrays cover nodes 0 .. n - 1, entry 0 the root (not read)."""

    def __init__(self, k, L, scoring, weighting, parent, is_leaf, desc, weight, device=0):
        parent = np.ascontiguousarray(parent, np.int32)
        n = len(parent)
        is_leaf = np.ascontiguousarray(is_leaf, np.uint8).reshape(n)
        desc = np.ascontiguousarray(desc, np.uint8).reshape(n, 32)
        weight = np.ascontiguousarray(weight, np.float64).reshape(n)
        self.h = lib.msl_vocab_create(device, k, L, scoring, weighting, n, ptr(parent), ptr(is_leaf), ptr(desc), ptr(weight))
        if not self.h:
            raise MslError(lib.msl_last_error().decode())
        self.device = device

    @classmethod
    def from_text(cls, path, device=0):
        """msl_vocab_load_text: DBoW2's text format (TemplatedVocabulary::loadFromTextFile)."""
        self = cls.__new__(cls)
        self.h = lib.msl_vocab_load_text(device, str(path).encode())
        if not self.h:
            raise MslError(lib.msl_last_error().decode())
        self.device = device
        return self

    def info(self):
        """{k, L, scoring, weighting, n_nodes, n_words, device}"""
        out = np.zeros(7, np.int32)
        check(lib.msl_vocab_info(self.h, ptr(out)), "msl_vocab_info")
        return dict(zip(("k", "L", "scoring", "weighting", "n_nodes", "n_words", "device"), (int(x) for x in out)))

    def close(self):
        if getattr(self, "h", None):
            lib.msl_vocab_destroy(self.h)
            self.h = None

    __del__ = close


def bow_match_params(nn_ratio=0.7, check_orientation=True):
    """msl_bow_match_params: ORBmatcher(nn_ratio, check_orientation) -- 0.7 at both tracking sites, 0.75 in Relocalization."""
    p = np.zeros(1, BOW_MATCH_PARAMS_DTYPE)
    p["nn_ratio"], p["check_orientation"] = nn_ratio, 1 if check_orientation else 0
    return p


def _counts(items, key):
    return np.array([len(x[key]) for x in items], np.int32)


def transform(vocab, frames, levelsup=4, cap=None, bow=True, handle=None, device=None):
    """ComputeBoW for every frame.  Returns one dict per frame: word (N,) i32, node (N,) i32 (-1 = stopped) and, with bow, bow_word (W,) i32
    ascending, bow_value (W,) f64."""
    F = len(frames)
    cap = cap or max(max(len(f["desc"]) for f in frames), 1)
    desc = pad(frames, "desc", cap, np.uint8, shape=(32,))
    n = _counts(frames, "desc")
    word = np.zeros((F, cap), np.int32); node = np.zeros((F, cap), np.int32)
    bw = np.zeros((F, cap), np.int32) if bow else None
    bv = np.zeros((F, cap), np.float64) if bow else None
    nw = np.zeros(F, np.int32) if bow else None
    dev = vocab.device if device is None else device
    if handle is not None:
        check(lib.msl_bow_transform(handle.h, vocab.h, F, cap, levelsup, ptr(desc), ptr(n), MSL_MEM_HOST, ptr(word), ptr(node), ptr(bw), ptr(bv),
                                    ptr(nw), MSL_MEM_HOST), "msl_bow_transform")
    else:
        check(lib.msl_bow_transform_batch(dev, vocab.h, F, cap, levelsup, ptr(desc), ptr(n), MSL_MEM_HOST, ptr(word), ptr(node), ptr(bw),
                                          ptr(bv), ptr(nw), MSL_MEM_HOST), "msl_bow_transform_batch")
    out = []
    for f in range(F):
        r = {"word": word[f, :n[f]].copy(), "node": node[f, :n[f]].copy()}
        if bow:
            r["bow_word"], r["bow_value"] = bw[f, :nw[f]].copy(), bv[f, :nw[f]].copy()
        out.append(r)
    return out


def to_maps(node, bow_word=None, bow_value=None):
    """The reference's containers from the ABI's arrays: (BowVector {word: value}, FeatureVector {node: [features ascending]})."""
    fv = {}
    for i, nd in enumerate(np.asarray(node).tolist()):
        if nd >= 0:
            fv.setdefault(nd, []).append(i)
    bv = {} if bow_word is None else {int(w): float(v) for w, v in zip(bow_word, bow_value)}
    return bv, dict(sorted(fv.items()))


def pack_match_by_bow(pairs, cap=None):
    """msl_match_by_bow's inputs in ABI order (kf_desc .. n_cur) and cap."""
    cap = cap or max(max(max(len(p["kf_desc"]), len(p["cur_desc"])) for p in pairs), 1)
    kps = np.zeros((len(pairs), cap), KEYPOINT_DTYPE)
    for f, p in enumerate(pairs):
        kps[f, :len(p["cur_angle"])]["angle"] = p["cur_angle"]
    arrays = [pad(pairs, "kf_desc", cap, np.uint8, shape=(32,)), pad(pairs, "kf_angle", cap, np.float32), pad(pairs, "kf_node", cap, np.int32, -1),
              pad(pairs, "kf_flags", cap, np.uint8), _counts(pairs, "kf_desc"), kps, pad(pairs, "cur_desc", cap, np.uint8, shape=(32,)),
              pad(pairs, "cur_node", cap, np.int32, -1), _counts(pairs, "cur_desc")]
    return cap, arrays


def match_by_bow(pairs, nn_ratio=0.7, check_orientation=True, cap=None, handle=None, device=0):
    """SearchByBoW(pKF, F) for every pair.  Returns (match lists: per frame feature the keyframe keypoint index or -1, nmatches)."""
    cap, arrays = pack_match_by_bow(pairs, cap)
    F = len(pairs)
    match = np.zeros((F, cap), np.int32); nm = np.zeros(F, np.int32)
    call("msl_match_by_bow", handle, device, F, cap, ptr(bow_match_params(nn_ratio, check_orientation)), *[ptr(a) for a in arrays], MSL_MEM_HOST,
         ptr(match), ptr(nm), MSL_MEM_HOST)
    return [match[f, :arrays[8][f]].copy() for f in range(F)], nm


def pack_lines_by_descriptor(pairs, lcap=None, klcap=None):
    """msl_match_lines_by_descriptor's inputs in ABI order (kf_ldesc .. n_cur_lines), lcap and klcap.  kf_line_xyz is None when no pair has kf_xyz."""
    lcap = lcap or max(max(len(p["cur_ldesc"]) for p in pairs), 1)
    klcap = klcap or max(max(len(p["kf_ldesc"]) for p in pairs), 1)
    xyz = None
    if all("kf_xyz" in p for p in pairs):
        xyz = pad(pairs, "kf_xyz", klcap, np.float64, shape=(6,))
    arrays = [pad(pairs, "kf_ldesc", klcap, np.uint8, shape=(32,)), pad(pairs, "kf_flags", klcap, np.uint8), xyz, _counts(pairs, "kf_ldesc"),
              pad(pairs, "cur_ldesc", lcap, np.uint8, shape=(32,)), _counts(pairs, "cur_ldesc")]
    return lcap, klcap, arrays


def match_lines_by_descriptor(pairs, lcap=None, klcap=None, pose_layout=False, handle=None, device=0):
    """SearchByDescriptor(pKF, F) for every pair.  Returns (match lists: per current line the keyframe line index or -1, nmatches) and, with
    pose_layout (every pair needs kf_xyz), also (line_xyz [pairs][lcap][6] f64, line_has [pairs][lcap] u8)."""
    lcap, klcap, arrays = pack_lines_by_descriptor(pairs, lcap, klcap)
    F = len(pairs)
    match = np.zeros((F, lcap), np.int32); nm = np.zeros(F, np.int32)
    lx = np.zeros((F, lcap, 6), np.float64) if pose_layout else None
    lh = np.zeros((F, lcap), np.uint8) if pose_layout else None
    call("msl_match_lines_by_descriptor", handle, device, F, lcap, klcap, *[ptr(a) for a in arrays], MSL_MEM_HOST, ptr(match), ptr(nm), ptr(lx),
         ptr(lh), MSL_MEM_HOST)
    res = [match[f, :arrays[5][f]].copy() for f in range(F)], nm
    return res + (lx, lh) if pose_layout else res


__all__ = ["Vocabulary", "bow_match_params", "transform", "to_maps", "match_by_bow", "match_lines_by_descriptor", "pack_match_by_bow",
           "pack_lines_by_descriptor", "TF_IDF", "TF", "IDF", "BINARY", "L1_NORM", "L2_NORM", "CHI_SQUARE", "KL", "BHATTACHARYYA",
           "DOT_PRODUCT"]

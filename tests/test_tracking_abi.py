"""The refusals of the thirteen Tracking entry points on the matcher handle (the two point searches, the two line searches, the two pose
optimisers, the three bag-of-words calls, the keyframe search, the relocalisation query, msl_pnp_ransac and msl_lines_3d), through the
device-indexed forms on host memory, which check before they touch a device: every limit, every params limit and every NULL is refused
with the field named, and the outputs keep their bytes.  One frame or pair of one keypoint or keyline, one local point or line, one level,
a 1 x 1 depth image.  No launch here (no GPU needed); with a device the unmodified scenes run."""
import ctypes as C

import numpy as np
import pytest

from tests import abi_refusals
from tests import pose_scenes as ps
from tests.abi_refusals import MSL_ERR_INVALID, both, declared, host_filled, put

TCW = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(np.float32)[None]      # [1][3][4]
SF = np.ones(1, np.float32)
LOG_SF = np.float32(np.log(1.2))
i32 = lambda *v: np.array(v, np.int32)


def _frame_params():
    from manhattanslam_amd._lib import FRAME_PARAMS_DTYPE
    p = np.zeros(1, FRAME_PARAMS_DTYPE)
    p["fx"], p["fy"], p["cx"], p["cy"], p["bf"], p["maxX"], p["maxY"] = 500, 500, 320, 240, 40, 640, 480
    return p


def _named(entry, params, arrays, **more):
    """The arrays a pack_* helper returns in argument order, by the names msl.h gives the pointers between `params` and `mem`."""
    from manhattanslam_amd import _header
    names = [n for t, n in _header.declarations(_header.text("msl.h"))[entry][1][1:] if t.endswith("*")]
    names = names[names.index("params") + 1:]
    return dict(zip(names, arrays), params=params, **more)


@pytest.fixture(scope="module")
def objects():
    """A vocabulary (L1 scoring) and an empty keyframe database on device 0.  On a machine without a device two words of host memory stand
    in for them: no check_x reads them, and without a device no call gets as far as launch_x, which would."""
    from manhattanslam_amd import bow, device_count, reloc
    if device_count() < 1:
        words = np.zeros(2, np.int64)
        yield C.c_void_p(words.ctypes.data), C.c_void_p(words.ctypes.data + 8)
        return
    voc = bow.Vocabulary(2, 1, bow.L1_NORM, bow.TF_IDF, i32(0, 0, 0), np.array([0, 1, 1], np.uint8), np.zeros((3, 32), np.uint8), np.ones(3))
    db = reloc.KeyFrameDatabase()
    yield C.c_void_p(voc.h), C.c_void_p(db.h)
    db.close(); voc.close()


@pytest.fixture(scope="module")
def scenes(objects):
    """entry -> (the int arguments, the input and in/out arrays, the outputs, the names of the in/out arrays)."""
    from manhattanslam_amd import KEYLINE_DTYPE, KEYPOINT_DTYPE, LINE_TRACK_DTYPE, LOCAL_TRACK_DTYPE, bow, line3d, match, pnp, pose, reloc
    from manhattanslam_amd._lib import pad
    voc, db = objects
    F = lambda *shape_dtype: host_filled(shape_dtype[:-1], shape_dtype[-1])
    fp = _frame_params()
    cur = dict(kps=np.zeros(1, KEYPOINT_DTYPE), un_xy=np.zeros((1, 2), np.float32), uright=np.full(1, -1, np.float32), grid_cell=np.zeros(1, np.int32),
               desc=np.zeros((1, 32), np.uint8), flags=np.zeros(1, np.uint8), held=np.zeros(1, np.uint8))
    pt = dict(xyz=np.array([[0, 0, 2]], np.float32), normal=np.array([[0, 0, -1]], np.float32), dist=np.array([[1, 4]], np.float32),
              desc=np.zeros((1, 32), np.uint8), flags=np.ones(1, np.uint8), octave=np.zeros(1, np.int32), angle=np.zeros(1, np.float32))
    kl = dict(kl=np.zeros(1, KEYLINE_DTYPE), desc=np.zeros((1, 32), np.uint8), flags=np.zeros(1, np.uint8))
    ln = dict(xyz=np.array([[-0.1, 0, 2, 0.1, 0, 2]], np.float64), normal=np.array([[0, 0, -1]], np.float64), dist=np.array([[1, 4]], np.float32),
              desc=np.zeros((1, 32), np.uint8), flags=np.ones(1, np.uint8), octave=np.zeros(1, np.int32))
    line_io = lambda: dict(line_xyz=np.zeros((1, 1, 6), np.float64), line_has=np.zeros((1, 1), np.uint8))
    s = {}
    e = "msl_match_by_projection"
    last = [pad([pt], "xyz", 1, np.float32, shape=(3,)), pad([pt], "desc", 1, np.uint8, shape=(32,)), pad([pt], "flags", 1, np.uint8),
            pad([pt], "octave", 1, np.int32), pad([pt], "angle", 1, np.float32), i32(1), match._rows3x4(TCW, 1), match._rows3x4(TCW, 1)]
    s[e] = (dict(n_pairs=1, cap=1), _named(e, match.match_params(fp, SF, 15.0), match._pack_cur([cur], 1) + last),
            dict(match_out=F(1, 1, np.int32), nmatches=F(1, np.int32)), ())
    e = "msl_match_local_points"
    cap, mcap, a = match.pack_local_points([cur], [pt], TCW)
    s[e] = (dict(n_frames=1, cap=cap, mcap=mcap), _named(e, match.local_match_params(fp, SF, 3.0, LOG_SF), a),
            dict(match_out=F(1, 1, np.int32), n_to_match=F(1, np.int32), nmatches=F(1, np.int32), in_view=F(1, 1, np.uint8),
                 track=F(1, 1, LOCAL_TRACK_DTYPE)), ())
    e = "msl_match_lines_by_projection"
    lcap, llcap, a = match.pack_lines_last([kl], [ln], TCW, TCW)
    s[e] = (dict(n_frames=1, lcap=lcap, llcap=llcap), _named(e, match.line_match_params(fp, SF, 15.0, LOG_SF), a, **line_io()),
            dict(match_out=F(1, 1, np.int32), nmatches=F(1, np.int32)), ("line_xyz", "line_has"))
    e = "msl_match_local_lines"
    lcap, mlcap, a = match.pack_local_lines([kl], [ln], TCW)
    s[e] = (dict(n_frames=1, lcap=lcap, mlcap=mlcap), _named(e, match.line_match_params(fp, SF, 1.0, LOG_SF), a, **line_io()),
            dict(match_out=F(1, 1, np.int32), n_to_match=F(1, np.int32), nmatches=F(1, np.int32), in_view=F(1, 1, np.uint8),
                 track=F(1, 1, LINE_TRACK_DTYPE)), ("line_xyz", "line_has"))
    fr = ps.empty(n=1, nl=1, m=1, x=1)
    fr["pt_ref"][0], fr["xyz"][0], fr["Tcw"] = 0, (0, 0, 2), TCW.reshape(12)
    (cap, xcap, lcap, pcap), a, io = pose.pack([fr])
    for e in ("msl_pose_optimize", "msl_pose_optimize_translation"):
        ins = _named(e, pose.pose_params(ps.params(nlevels=1)), a, outlier=io[0], line_outlier=io[1], plane_outlier=io[2])
        if e.endswith("translation"):
            ins["Rcw"] = np.eye(3, dtype=np.float32).reshape(1, 9)
        s[e] = (dict(n_frames=1, cap=cap, xcap=xcap, lcap=lcap, pcap=pcap), ins, dict(Tcw_out=F(1, 12, np.float32), n_good=F(1, np.int32)),
                ("outlier", "line_outlier", "plane_outlier"))
    s["msl_bow_transform"] = (dict(n_frames=1, cap=1, levelsup=0), dict(v=voc, desc=np.zeros((1, 1, 32), np.uint8), n_desc=i32(1)),
                              dict(word_out=F(1, 1, np.int32), node_out=F(1, 1, np.int32), bow_word=F(1, 1, np.int32), bow_value=F(1, 1, np.float64),
                                   n_words=F(1, np.int32)), ())
    e = "msl_match_by_bow"
    pair = dict(kf_desc=np.zeros((1, 32), np.uint8), kf_angle=np.zeros(1, np.float32), kf_node=i32(0), kf_flags=np.ones(1, np.uint8),
                cur_angle=np.zeros(1, np.float32), cur_desc=np.zeros((1, 32), np.uint8), cur_node=i32(0))
    cap, a = bow.pack_match_by_bow([pair])
    s[e] = (dict(n_pairs=1, cap=cap), _named(e, bow.bow_match_params(), a), dict(match_out=F(1, 1, np.int32), nmatches=F(1, np.int32)), ())
    e = "msl_match_lines_by_descriptor"
    lpair = dict(kf_ldesc=np.zeros((1, 32), np.uint8), kf_flags=np.ones(1, np.uint8), kf_xyz=ln["xyz"], cur_ldesc=np.zeros((1, 32), np.uint8))
    lcap, klcap, a = bow.pack_lines_by_descriptor([lpair])
    names = ("kf_ldesc", "kf_line_flags", "kf_line_xyz", "n_kf_lines", "cur_ldesc", "n_cur_lines")      # no params to count from
    s[e] = (dict(n_pairs=1, lcap=lcap, klcap=klcap), dict(zip(names, a), line_xyz=np.zeros((1, 1, 6), np.float64)),
            dict(match_out=F(1, 1, np.int32), nmatches=F(1, np.int32), line_has=F(1, 1, np.uint8)), ("line_xyz",))
    e = "msl_match_keyframe_points"
    cap, kcap, a = reloc.pack_keyframe_points([cur], [pt], TCW)
    s[e] = (dict(n_pairs=1, cap=cap, kcap=kcap), _named(e, reloc.keyframe_match_params(fp, SF, 10.0, 100, LOG_SF), a),
            dict(match_out=F(1, 1, np.int32), nmatches=F(1, np.int32)), ())
    s["msl_reloc_candidates"] = (dict(n_frames=1, cap=1, ccap=1),
                                 dict(db=db, voc=voc, bow_word=i32(0).reshape(1, 1), bow_value=np.ones((1, 1)), n_words=i32(1), covis=reloc.pack_covis([], 0)),
                                 dict(cand_out=F(1, 1, np.int32), n_cand=F(1, np.int32), words_out=F(1, 1, np.int32), score_out=F(1, 1, np.float32)), ())
    e = "msl_pnp_ransac"
    cap, kcap, a = pnp.pack_pnp([dict(octave=i32(0), un_xy=np.zeros((1, 2), np.float32), match=i32(0), xyz=pt["xyz"], seed=1)])
    s[e] = (dict(n_pairs=1, cap=cap, kcap=kcap), _named(e, pnp.pnp_params(500, 500, 320, 240, [1.0]), a),
            dict(Tcw_out=F(1, 12, np.float32), inlier=F(1, 1, np.uint8), pt_ref_out=F(1, 1, np.int32), n_inliers=F(1, np.int32), status=F(1, np.int32)), ())
    lcap, W, H, a = line3d.pack_lines([dict(line_ends=np.zeros((1, 4), np.float32), depth=np.ones((1, 1), np.float32), Tcw=TCW[0], seed=[1])])
    s["msl_lines_3d"] = (dict(n_frames=1, lcap=lcap, order=line3d.DEPTH_ORDER, width=W, height=H, depth_row_stride=4 * W, depth_frame_stride=4 * W * H),
                         dict(a, params=line3d.line3d_params(500, 500, 320, 240)),
                         dict(line_depth=F(1, 1, 2, np.float32), line_xyz=F(1, 1, 6, np.float64), line_ok=F(1, 1, np.uint8), line_new=F(1, 1, np.uint8),
                              n_support=F(1, 1, np.int32), n_new=F(1, np.int32)), ())
    return s


ENTRIES = ("msl_bow_transform", "msl_lines_3d", "msl_match_by_bow", "msl_match_by_projection", "msl_match_keyframe_points",
           "msl_match_lines_by_descriptor", "msl_match_lines_by_projection", "msl_match_local_lines", "msl_match_local_points", "msl_pnp_ransac",
           "msl_pose_optimize", "msl_pose_optimize_translation", "msl_reloc_candidates")


def call(scenes, entry, **over):
    """abi_refusals.call on the scene of `entry`, on a copy of its outputs: with a device an accepted call writes them."""
    ints, ins, out, inout = scenes[entry]
    return abi_refusals.call(entry, ints, ins, {k: v.copy() for k, v in out.items()}, inout=inout, **over)


def refused(scenes, entry, **over):
    rc, msg = call(scenes, entry, **over)
    assert rc == MSL_ERR_INVALID, (entry, over, rc, msg)
    return msg


below = lambda field: [(field, 0, f"{field} 0 below 1"), (field, -2, f"{field} -2 below 1")]
POSE_LIMITS = below("n_frames") + both("cap", 8192) + both("xcap", 32768) + both("lcap", 256) + both("pcap", 64)
IMAGE = "depth image %d x %d with strides 4 / 4 bytes is not a float image"   # width, height and the two strides share one message
LIMITS = {
    "msl_match_by_projection": below("n_pairs") + both("cap", 8192),
    "msl_match_local_points": below("n_frames") + both("cap", 8192) + both("mcap", 32768),
    "msl_match_lines_by_projection": below("n_frames") + both("lcap", 256) + both("llcap", 256),
    "msl_match_local_lines": below("n_frames") + both("lcap", 256) + both("mlcap", 32768),
    "msl_pose_optimize": POSE_LIMITS, "msl_pose_optimize_translation": POSE_LIMITS,
    "msl_bow_transform": below("n_frames") + both("cap", 8192),
    "msl_match_by_bow": below("n_pairs") + both("cap", 8192),
    "msl_match_lines_by_descriptor": below("n_pairs") + both("lcap", 256) + both("klcap", 256),
    "msl_match_keyframe_points": below("n_pairs") + both("cap", 8192) + both("kcap", 8192),
    "msl_reloc_candidates": below("n_frames") + below("cap") + below("ccap"),                      # cap and ccap have no upper limit
    "msl_pnp_ransac": below("n_pairs") + both("cap", 8192) + both("kcap", 32768),
    "msl_lines_3d": below("n_frames") + both("lcap", 256) + [
        ("order", -1, "order -1 is not an MSL_LINE3D_* value"), ("order", 3, "order 3 is not an MSL_LINE3D_* value"),
        ("width", 0, IMAGE % (0, 1)), ("height", 0, IMAGE % (1, 0))],
}
UNLIMITED = {"msl_bow_transform": {"levelsup"}}                           # an int argument that every value of is accepted
# the limits on fields of `params`
FRAME = both("nlevels", 16) + [("maxX", 0, "image bounds minX 0 .. maxX 0 are empty"), ("minX", np.nan, "image bounds minX nan .. maxX 640 are empty"),
                               ("maxY", -1, "image bounds minY 0 .. maxY -1 are empty"), ("fx", 0, "fx is 0")]
LOG_SCALE = [("log_scale_factor", 0, "log_scale_factor 0 is not above 0"), ("log_scale_factor", np.nan, "log_scale_factor nan is not above 0")]
PARAM_LIMITS = {
    "msl_match_by_projection": FRAME, "msl_match_lines_by_projection": FRAME,
    "msl_match_local_points": FRAME + LOG_SCALE, "msl_match_local_lines": FRAME + LOG_SCALE,
    "msl_match_keyframe_points": FRAME + LOG_SCALE + [("orb_dist", -1, "orb_dist -1 outside 0 .. 255"), ("orb_dist", 256, "orb_dist 256 outside 0 .. 255")],
    "msl_pose_optimize": both("nlevels", 16), "msl_pose_optimize_translation": both("nlevels", 16),
    "msl_pnp_ransac": both("nlevels", 16) + both("max_iterations", 1024) + [
        ("min_set", 3, "min_set 3 (only 4, the reference's one use, is built)"), ("min_set", 5, "min_set 5 (only 4, the reference's one use, is built)"),
        ("n_iterations", -1, "n_iterations -1 outside 0 .. 1024"), ("n_iterations", 1025, "n_iterations 1025 outside 0 .. 1024")],
    "msl_lines_3d": both("max_samples", 127) + [("max_iterations", -1, "max_iterations -1 outside 0 .. 64"),
                                                ("max_iterations", 65, "max_iterations 65 outside 0 .. 64"), ("min_points", 1, "min_points 1 below 2")],
}


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_limit_is_refused_with_the_field_named(scenes, entry):
    assert {l[0] for l in LIMITS[entry]} | UNLIMITED.get(entry, set()) == set(declared(entry)[0])
    for field, value, msg in LIMITS[entry]:
        assert refused(scenes, entry, **{field: value}) == f"{entry}: {msg}"
    for field, value, msg in PARAM_LIMITS.get(entry, ()):
        assert refused(scenes, entry, params=put(field, value)) == f"{entry}: {msg}"


def test_the_strides_of_msl_lines_3d_are_refused_with_the_image_named(scenes):
    """A row shorter than `width` floats, strides that are no multiple of a float, and frames that overlap."""
    e = "msl_lines_3d"
    msg = e + ": depth image 1 x 1 with strides %d / %d bytes is not a float image"
    assert refused(scenes, e, depth_row_stride=3) == msg % (3, 4)
    assert refused(scenes, e, depth_row_stride=6) == msg % (6, 4)
    assert refused(scenes, e, depth_frame_stride=2) == msg % (4, 2)
    assert refused(scenes, e, n_frames=2, depth_row_stride=8) == msg % (8, 4)


# the arrays an entry may be called without
OPTIONAL = {"msl_match_local_points": ["in_view", "track"], "msl_match_lines_by_projection": ["line_xyz", "line_has"],
            "msl_match_local_lines": ["in_view", "track", "line_xyz", "line_has"], "msl_pose_optimize_translation": ["Rcw"],
            "msl_reloc_candidates": ["covis", "words_out", "score_out"], "msl_lines_3d": ["line_flags"]}
# the arrays that are given all or none, or that another one makes required: each has an assertion of its own below
CONDITIONAL = {"msl_bow_transform": ["bow_word", "bow_value", "n_words"], "msl_match_lines_by_descriptor": ["kf_line_xyz", "line_xyz", "line_has"]}
ON_THE_HANDLE = {"msl_bow_transform": ["v"]}                              # compared with the handle's device: launch_x's to refuse
POINTERS = {"msl_match_by_projection": 17, "msl_match_local_points": 20, "msl_match_lines_by_projection": 15, "msl_match_local_lines": 19,
            "msl_pose_optimize": 21, "msl_pose_optimize_translation": 22, "msl_bow_transform": 8, "msl_match_by_bow": 12,
            "msl_match_lines_by_descriptor": 10, "msl_match_keyframe_points": 16, "msl_reloc_candidates": 10, "msl_pnp_ransac": 12,
            "msl_lines_3d": 13}


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_null_is_refused_with_the_field_named(scenes, entry):
    pointers = declared(entry)[1]
    free = OPTIONAL.get(entry, []) + CONDITIONAL.get(entry, []) + ON_THE_HANDLE.get(entry, [])
    assert len(pointers) == POINTERS[entry] and set(free) <= set(pointers)
    for n in pointers:
        if n not in free:
            assert refused(scenes, entry, **{n: None}) == f"{entry}: {n} is NULL"
    for n in OPTIONAL.get(entry, []):
        assert call(scenes, entry, **{n: None})[0] != MSL_ERR_INVALID, n


def test_the_vector_of_msl_bow_transform_is_given_all_or_none(scenes):
    e = "msl_bow_transform"
    for n in CONDITIONAL[e]:
        assert refused(scenes, e, **{n: None}) == f"{e}: bow_word, bow_value and n_words are given all or none"
    assert refused(scenes, e, bow_word=None, n_words=None) == f"{e}: bow_word, bow_value and n_words are given all or none"
    assert call(scenes, e, bow_word=None, bow_value=None, n_words=None)[0] != MSL_ERR_INVALID
    rc, msg = call(scenes, e, v=None)                                       # no device: never looked at; with one: launch_transform's refusal
    assert rc != MSL_ERR_INVALID or msg == f"{e}: null vocabulary"


def test_the_pose_layout_of_msl_match_lines_by_descriptor(scenes):
    e = "msl_match_lines_by_descriptor"
    assert refused(scenes, e, line_xyz=None) == f"{e}: line_xyz and line_has are given together"
    assert refused(scenes, e, line_has=None) == f"{e}: line_xyz and line_has are given together"
    assert refused(scenes, e, kf_line_xyz=None) == f"{e}: kf_line_xyz is NULL"
    assert call(scenes, e, kf_line_xyz=None, line_xyz=None, line_has=None)[0] != MSL_ERR_INVALID
    assert call(scenes, e, line_xyz=None, line_has=None)[0] != MSL_ERR_INVALID


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_smallest_scene_is_not_refused(scenes, entry):
    """Unmodified: MSL_ERR_NO_DEVICE without a device, MSL_OK with one."""
    from manhattanslam_amd import device_count
    rc, msg = call(scenes, entry)
    assert rc != MSL_ERR_INVALID and (rc == 0 or device_count() < 1), (rc, msg)


def test_the_handle_forms_refuse_a_null_handle():
    from manhattanslam_amd import _lib
    for entry in ENTRIES:
        args = [0 if t in (C.c_int, C.c_uint, C.c_size_t) else None for t in _lib.SIGNATURES[entry][1][1:]]
        assert getattr(_lib.lib, entry)(None, *args) == MSL_ERR_INVALID
        assert _lib.lib.msl_last_error().decode() == f"{entry}: h is NULL"

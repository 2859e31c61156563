"""The refusals of the seven LocalMapping entry points that triangulate, fuse and refresh (msl_refresh_map_points, msl_covisibility,
msl_fuse_candidates, msl_fuse_map_points, msl_fuse_map_lines, msl_refresh_map_lines, msl_triangulate_new_points), through the device-indexed
forms on host memory, which check before they touch a device: every limit, every NULL and every index defect of a host-memory call is
refused with the field named, and the outputs keep their bytes.  Two keyframes of one feature, one point or line, one item, one list of one
candidate.  No launch (no GPU needed)."""
import numpy as np
import pytest

from tests import abi_refusals
from tests.abi_refusals import both, declared as _declared, host_filled, put

TCW = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(np.float32)
SF = np.ones(1, np.float32)
OBS = dict(obs_off=np.array([0, 2], np.int32), obs_kf=np.array([0, 1], np.int32), obs_idx=np.zeros(2, np.int32))
TABLE = dict(n_tab=2, cap=1, n_pts=1, n_items=1)
LINE_TABLE = dict(n_tab=2, klcap=1, n_lines=1, n_items=1)


def _refused(fn, *a, **kw):
    """The library's message when fn(*a, **kw) is refused as an invalid argument."""
    from manhattanslam_amd._lib import MslError, lib
    with pytest.raises(MslError, match=r"failed \(-1\)"):
        fn(*a, **kw)
    return lib.msl_last_error().decode()


def _points():
    from manhattanslam_amd import KEYPOINT_DTYPE, fuse
    kf = dict(kps_un=np.zeros(1, KEYPOINT_DTYPE), uright=np.full(1, -1, np.float32), grid_cell=np.zeros(1, np.int32), desc=np.zeros((1, 32), np.uint8),
              held_id=np.full(1, -1, np.int32), Tcw=TCW)
    pts = dict(xyz=np.array([[0, 0, 2]], np.float32), normal=np.array([[0, 0, 1]], np.float32), dist=np.array([[1, 4]], np.float32),
               desc=np.zeros((1, 32), np.uint8), flags=np.ones(1, np.uint8), nobs=np.ones(1, np.int32))
    return fuse.fuse_params(500, 500, 320, 240, 40, 0, 640, 0, 480, SF, SF, np.float32(np.log(1.2))), [kf, kf], pts


def _lines():
    from manhattanslam_amd import KEYLINE_DTYPE, linefuse
    kf = dict(kl=np.zeros(1, KEYLINE_DTYPE), ldesc=np.zeros((1, 32), np.uint8), held_id=np.full(1, -1, np.int32), Tcw=TCW)
    lns = dict(xyz=np.array([[-0.1, 0, 2, 0.1, 0, 2]], np.float64), normal=np.array([[0, 0, 1]], np.float64), dist=np.array([[1, 4]], np.float32),
               desc=np.zeros((1, 32), np.uint8), flags=np.ones(1, np.uint8), nobs=np.ones(1, np.int32))
    return linefuse.line_fuse_params(500, 500, 320, 240, 0, 640, 0, 480, SF, np.float32(np.log(1.2))), [kf, kf], lns


def _triangulation():
    from manhattanslam_amd import KEYPOINT_DTYPE, triangulate
    kf = dict(kps_un=np.zeros(1, KEYPOINT_DTYPE), raw_xy=np.zeros((1, 2), np.float32), uright=np.full(1, -1, np.float32), depth=np.full(1, -1, np.float32),
              desc=np.zeros((1, 32), np.uint8), node=np.zeros(1, np.int32), held=np.zeros(1, np.uint8), Tcw=TCW)
    return triangulate.triangulate_params(500, 500, 320, 240, 40, SF, SF, 1.2), [kf, kf]


# ---- the refusals compared in full, through the wrappers -------------------------------------------------------------------------------------
def test_list_refusals_of_the_batch_forms():
    from manhattanslam_amd import fuse, linefuse
    prm, table, pts = _points()
    assert _refused(fuse.fuse_map_points, prm, table, pts, [(1, 0)], [[1]]) == "msl_fuse_map_points: list 0 entry 0 is point 1 of 1"
    assert _refused(fuse.fuse_map_points, prm, table, pts, [(2, 0)], [[0]]) == "msl_fuse_map_points: item 0 names keyframe 2 of 2 or list 0 of 1"
    prm, table, lns = _lines()
    assert _refused(linefuse.fuse_map_lines, prm, table, lns, [(1, 0)], [[1]]) == "msl_fuse_map_lines: list 0 entry 0 is line 1 of 1"
    assert _refused(linefuse.fuse_map_lines, prm, table, lns, [(1, 1)], [[0]]) == "msl_fuse_map_lines: item 0 names keyframe 1 of 2 or list 1 of 1"


def test_neighbour_and_target_refusals_of_the_batch_forms():
    from manhattanslam_amd import KEYPOINT_DTYPE, fuse, triangulate
    kf = dict(kps_un=np.zeros(1, KEYPOINT_DTYPE), raw_xy=np.zeros((1, 2), np.float32), uright=np.full(1, -1, np.float32), depth=np.full(1, -1, np.float32),
              desc=np.zeros((1, 32), np.uint8), node=np.zeros(1, np.int32), held=np.zeros(1, np.uint8), Tcw=TCW)
    prm = triangulate.triangulate_params(500, 500, 320, 240, 40, SF, SF, 1.2)
    assert _refused(triangulate.triangulate_new_points, prm, [kf, kf], [(0, [0])]) == (
        "msl_triangulate_new_points: item 0 names a keyframe outside the table of 2, repeats a neighbour, lists its current keyframe as a "
        "neighbour, or has n_neigh outside 0 .. 1")
    _, table, pts = _points()
    assert _refused(fuse.fuse_candidates, table, pts, [[2]]) == (
        "msl_fuse_candidates: item 0 names a keyframe outside the table of 2, or has n_targets outside 0 .. 1")


# ---- every entry on the raw ABI ---------------------------------------------------------------------------------------------------------------
def _scenes():
    """entry -> (the int arguments, the arrays before `mem`, outputs(shape) -> the arrays after it: None for an optional one)."""
    from manhattanslam_amd import fuse, linefuse, mappoint, triangulate
    i32 = lambda *v: np.array(v, np.int32)
    prm, kfs, pts = _points()
    _, t = fuse.pack_table(kfs)
    _, p = fuse.pack_points(pts)
    lprm, lkfs, lns = _lines()
    _, lt = linefuse.pack_line_table(lkfs)
    _, lp = linefuse.pack_lines(lns)
    tprm, tkfs = _triangulation()
    _, tt = triangulate.pack_table(tkfs)
    lists = dict(tgt=i32(1), list=i32(0), cand=i32(0).reshape(1, 1), n_cand=i32(1))
    fuse_out = lambda sh: fuse.outputs(sh["n_items"], sh["lcap"], host_filled)
    return {
        "msl_refresh_map_points": (dict(TABLE, n_obs_total=2, what=3),
                                   dict(t, **OBS, params=mappoint.refresh_params(SF), kf_flags=np.ones(2, np.uint8), pt_xyz=p["pt_xyz"],
                                        pt_flags=p["pt_flags"], pt_ref=i32(0), ids=i32(0)),
                                   lambda sh: dict(mappoint.refresh_outputs(sh["n_items"], host_filled), pt_desc=None, pt_normal=None, pt_dist=None)),
        "msl_covisibility": (dict(TABLE, n_obs_total=2, ccap=1, th=15),
                             dict(OBS, held_id=i32(0, 0).reshape(2, 1), n_kps=t["n_kps"], pt_flags=p["pt_flags"], kf=i32(0)),
                             lambda sh: mappoint.covisibility_outputs(sh["n_items"], sh["n_tab"], sh["ccap"], host_filled)),
        "msl_fuse_candidates": (dict(TABLE, tcap=1, lcap=1),
                                dict(held_id=t["held_id"], n_kps=t["n_kps"], pt_flags=p["pt_flags"], targets=i32(1).reshape(1, 1), n_targets=i32(1)),
                                lambda sh: dict(cand=host_filled((sh["n_items"], sh["lcap"]), np.int32), n_cand=host_filled((sh["n_items"],), np.int32))),
        "msl_fuse_map_points": (dict(TABLE, n_lists=1, lcap=1), dict(t, **p, **lists, params=prm), fuse_out),
        "msl_fuse_map_lines": (dict(LINE_TABLE, n_lists=1, lcap=1), dict(lt, **{k: lp[k] for k in linefuse.LINE_KEYS}, **lists, params=lprm), fuse_out),
        "msl_refresh_map_lines": (dict(LINE_TABLE, n_obs_total=2),
                                  dict(OBS, params=mappoint.refresh_params(SF), kl=lt["kl"], n_kl=lt["n_kl"], Tcw=lt["Tcw"], ln_xyz=lp["ln_xyz"],
                                       ln_flags=lp["ln_flags"], ln_ref=i32(0), ids=i32(0)),
                                  lambda sh: dict(linefuse.refresh_outputs(sh["n_items"], host_filled), ln_normal=None, ln_dist=None)),
        "msl_triangulate_new_points": (dict(n_tab=2, cap=1, n_items=1, ncap=1),
                                       dict(tt, params=tprm, cur=i32(0), neigh=i32(1).reshape(1, 1), n_neigh=i32(1)),
                                       lambda sh: triangulate.outputs(sh["n_items"], sh["ncap"], sh["cap"], host_filled)),
    }


@pytest.fixture(scope="module")
def scenes():
    return _scenes()


ENTRIES = ("msl_covisibility", "msl_fuse_candidates", "msl_fuse_map_lines", "msl_fuse_map_points", "msl_refresh_map_lines", "msl_refresh_map_points",
           "msl_triangulate_new_points")


def refused(scenes, entry, shape=None, **over):
    """abi_refusals.refused on the scene of `entry`.  shape: the int arguments the outputs are sized for, when the replaced arrays describe
    a larger call."""
    ints, ins, outputs = scenes[entry]
    return abi_refusals.refused(entry, ints, ins, outputs(dict(ints, **(shape or {}))), **over)


POINT_TABLE_LIMITS = both("n_tab", 4096) + both("cap", 8192) + both("n_pts", 1 << 20)
LINE_TABLE_LIMITS = both("n_tab", 4096) + both("klcap", 256) + both("n_lines", 1 << 20)
ITEM_LIMITS = both("n_items", 4096) + both("lcap", 65536)
OBS_LIMIT = [("n_obs_total", -1, "n_obs_total -1 below 0")]
LIMITS = {
    "msl_refresh_map_points": POINT_TABLE_LIMITS + OBS_LIMIT + both("n_items", 1, "n_pts = 1") + [
        ("what", 0, "what 0 outside the mask MSL_REFRESH_DESC | MSL_REFRESH_NORMAL"), ("what", 4, "what 4 outside the mask MSL_REFRESH_DESC | MSL_REFRESH_NORMAL")],
    "msl_covisibility": POINT_TABLE_LIMITS + OBS_LIMIT + both("n_items", 2, "n_tab = 2") + both("ccap", 2, "n_tab = 2"),
    "msl_fuse_candidates": POINT_TABLE_LIMITS + ITEM_LIMITS + both("tcap", 64),
    "msl_fuse_map_points": POINT_TABLE_LIMITS + ITEM_LIMITS + [("n_lists", 0, "n_lists 0 below 1")],
    "msl_fuse_map_lines": LINE_TABLE_LIMITS + ITEM_LIMITS + [("n_lists", 0, "n_lists 0 below 1")],
    "msl_refresh_map_lines": LINE_TABLE_LIMITS + OBS_LIMIT + both("n_items", 1, "n_lines = 1"),
    "msl_triangulate_new_points": both("n_tab", 4096) + both("cap", 8192) + both("ncap", 16) + [
        ("n_items", 0, "n_items 0 below 1"), ("n_items", 65536, "n_items 65536 above 65535")],
}
UNLIMITED = {"msl_covisibility": {"th"}}                                  # an int argument that every value of is accepted
# the limits on fields of `params`
PARAM_LIMITS = {
    "msl_refresh_map_points": both("nlevels", 16), "msl_refresh_map_lines": both("nlevels", 16), "msl_triangulate_new_points": both("nlevels", 16),
    "msl_fuse_map_points": both("nlevels", 16) + [("th_low", -1, "th_low -1 outside 0 .. 255"), ("th_low", 256, "th_low 256 outside 0 .. 255")],
    "msl_fuse_map_lines": both("nlevels", 16) + [("th_low", -1, "th_low -1 outside 0 .. 256"), ("th_low", 257, "th_low 257 outside 0 .. 256")],
}


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_limit_is_refused_with_the_field_named(scenes, entry):
    assert {l[0] for l in LIMITS[entry]} | UNLIMITED.get(entry, set()) == set(_declared(entry)[0])
    for field, value, msg in LIMITS[entry]:
        assert refused(scenes, entry, **{field: value}) == f"{entry}: {msg}"
    for field, value, msg in PARAM_LIMITS.get(entry, ()):
        assert refused(scenes, entry, params=put(field, value)) == f"{entry}: {msg}"


# the arrays an entry may be called without: the table rows of the two refreshes
OPTIONAL = {"msl_refresh_map_points": ["pt_desc", "pt_normal", "pt_dist"], "msl_refresh_map_lines": ["ln_normal", "ln_dist"]}
POINTERS = {"msl_refresh_map_points": 22, "msl_covisibility": 10, "msl_fuse_candidates": 7, "msl_fuse_map_points": 23, "msl_fuse_map_lines": 21,
            "msl_refresh_map_lines": 16, "msl_triangulate_new_points": 24}


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_null_is_refused_with_the_field_named(scenes, entry):
    pointers = _declared(entry)[1]
    assert len(pointers) == POINTERS[entry] and set(OPTIONAL.get(entry, ())) <= set(pointers)
    for n in pointers:
        if n not in OPTIONAL.get(entry, ()):
            assert refused(scenes, entry, **{n: None}) == f"{entry}: {n} is NULL"


def test_what_decides_the_arrays_msl_refresh_map_points_requires(scenes):
    """With MSL_REFRESH_DESC alone kps_un, Tcw, pt_xyz and pt_ref may be NULL: such a call is refused for its one defect, not for them; and
    `what` is tested before any pointer."""
    e = "msl_refresh_map_points"
    free = dict(kps_un=None, Tcw=None, pt_xyz=None, pt_ref=None)
    assert refused(scenes, e, what=1, n_items=0, **free) == f"{e}: n_items 0 outside 1 .. n_pts = 1"
    assert refused(scenes, e, what=1, ids=put(0, 1), **free) == f"{e}: ids[0] is 1 of 1"
    assert refused(scenes, e, what=1, params=put("nlevels", 17), ids=put(0, -1)) == f"{e}: ids[0] is -1 of 1"   # nlevels is UpdateNormalAndDepth's
    assert refused(scenes, e, what=2, Tcw=None) == f"{e}: Tcw is NULL"
    assert refused(scenes, e, what=0, desc=None) == f"{e}: what 0 outside the mask MSL_REFRESH_DESC | MSL_REFRESH_NORMAL"


def _observation_defects(refuse, e, count):
    """The defects of the observation table (count: the name of the keyframes' counts where the entry reads obs_idx, else None)."""
    assert refuse(obs_off=put(0, -1)) == f"{e}: obs_off[0] is -1, below 0"
    assert refuse(obs_off=put(0, 3)) == f"{e}: obs_off descends at point 0 (2 after 3)"
    assert refuse(obs_off=put(1, 1)) == f"{e}: obs_off[n_pts] is 1, n_obs_total 2"
    assert refuse(obs_kf=put(1, 2)) == f"{e}: obs_kf[1] is keyframe 2 of 2"
    assert refuse(obs_kf=put(0, -1)) == f"{e}: obs_kf[0] is keyframe -1 of 2"
    if count:
        assert refuse(obs_idx=put(1, 1)) == f"{e}: obs_idx[1] is keypoint 1 of 1 in keyframe 1"
        assert refuse(obs_idx=put(0, -1)) == f"{e}: obs_idx[0] is keypoint -1 of 1 in keyframe 0"
        assert refuse(**{count: put(1, 0)}) == f"{e}: obs_idx[1] is keypoint 0 of 0 in keyframe 1"


def test_index_defects_of_the_refreshes_and_the_covisibility(scenes):
    i32 = lambda *v: np.array(v, np.int32)
    two = dict(obs_off=i32(0, 2, 2), ids=i32(0, 0))                        # a second point without observations, and the first named twice
    e = "msl_refresh_map_points"
    refuse = lambda **over: refused(scenes, e, **over)
    _observation_defects(refuse, e, "n_kps")
    assert refuse(ids=put(0, 1)) == f"{e}: ids[0] is 1 of 1"
    assert refuse(ids=put(0, -1)) == f"{e}: ids[0] is -1 of 1"
    assert refuse(shape=dict(n_items=2), n_pts=2, n_items=2, pt_xyz=np.zeros((2, 3), np.float32), pt_flags=np.ones(2, np.uint8), pt_ref=i32(0, 0),
                  **two) == f"{e}: ids holds 0 twice"
    assert refuse(pt_ref=put(0, 2)) == f"{e}: pt_ref[0] is keyframe 2 of 2"
    assert refuse(pt_ref=put(0, -1)) == f"{e}: pt_ref[0] is keyframe -1 of 2"
    e = "msl_refresh_map_lines"
    refuse = lambda **over: refused(scenes, e, **over)
    _observation_defects(refuse, e, "n_kl")
    assert refuse(ids=put(0, 1)) == f"{e}: ids[0] is 1 of 1"
    assert refuse(ids=put(0, -1)) == f"{e}: ids[0] is -1 of 1"
    assert refuse(shape=dict(n_items=2), n_lines=2, n_items=2, ln_xyz=np.zeros((2, 6), np.float64), ln_flags=np.ones(2, np.uint8), ln_ref=i32(0, 0),
                  **two) == f"{e}: ids holds 0 twice"
    e = "msl_covisibility"
    refuse = lambda **over: refused(scenes, e, **over)
    _observation_defects(refuse, e, None)
    assert refuse(kf=put(0, 2)) == f"{e}: kf[0] is 2 of 2"
    assert refuse(kf=put(0, -1)) == f"{e}: kf[0] is -1 of 2"


def test_index_defects_of_the_fusions_and_the_triangulation(scenes):
    i32 = lambda *v: np.array(v, np.int32)
    for e, noun in (("msl_fuse_map_points", "point"), ("msl_fuse_map_lines", "line")):
        refuse = lambda **over: refused(scenes, e, **over)
        assert refuse(tgt=put(0, 2)) == f"{e}: item 0 names keyframe 2 of 2 or list 0 of 1"
        assert refuse(tgt=put(0, -1)) == f"{e}: item 0 names keyframe -1 of 2 or list 0 of 1"
        assert refuse(list=put(0, 1)) == f"{e}: item 0 names keyframe 1 of 2 or list 1 of 1"
        assert refuse(list=put(0, -1)) == f"{e}: item 0 names keyframe 1 of 2 or list -1 of 1"
        assert refuse(n_cand=put(0, 2)) == f"{e}: list 0 has n_cand 2 outside 0 .. 1"
        assert refuse(n_cand=put(0, -1)) == f"{e}: list 0 has n_cand -1 outside 0 .. 1"
        assert refuse(cand=put((0, 0), 1)) == f"{e}: list 0 entry 0 is {noun} 1 of 1"
        assert refuse(cand=put((0, 0), -2)) == f"{e}: list 0 entry 0 is {noun} -2 of 1"
        assert refuse(shape=dict(lcap=2), lcap=2, cand=i32(0, 0).reshape(1, 2), n_cand=i32(2)) == (
            f"{e}: list 0 holds {noun} 0 twice (pass -1 for a later duplicate)")
    e = "msl_fuse_candidates"
    msg = f"{e}: item 0 names a keyframe outside the table of 2, or has n_targets outside 0 .. 1"
    for over in (dict(targets=put((0, 0), 2)), dict(targets=put((0, 0), -1)), dict(n_targets=put(0, 2)), dict(n_targets=put(0, -1))):
        assert refused(scenes, e, **over) == msg
    e = "msl_triangulate_new_points"
    msg = (f"{e}: item 0 names a keyframe outside the table of 2, repeats a neighbour, lists its current keyframe as a neighbour, or has n_neigh "
           "outside 0 .. %d")
    for over in (dict(cur=put(0, 2)), dict(cur=put(0, -1)), dict(neigh=put((0, 0), 2)), dict(neigh=put((0, 0), -1)), dict(neigh=put((0, 0), 0)),
                 dict(n_neigh=put(0, 2)), dict(n_neigh=put(0, -1))):
        assert refused(scenes, e, **over) == msg % 1
    assert refused(scenes, e, shape=dict(ncap=2), ncap=2, neigh=i32(1, 1).reshape(1, 2), n_neigh=i32(2)) == msg % 2


def test_the_handle_forms_refuse_a_null_handle():
    import ctypes as C
    from manhattanslam_amd import _lib
    for entry in ENTRIES:
        args = [0 if t in (C.c_int, C.c_uint) else None for t in _lib.SIGNATURES[entry][1][1:]]
        assert getattr(_lib.lib, entry)(None, *args) == -1
        assert _lib.lib.msl_last_error().decode() == f"{entry}: h is NULL"

"""msl_triangulate_new_points, msl_fuse_candidates, msl_fuse_map_points, msl_fuse_map_lines, msl_refresh_map_points, msl_refresh_map_lines
and msl_covisibility on the GPU at the limits include/msl.h accepts, on the scenes of tests/search_limit_scenes.py (its docstring lists the
cases and the pairs of limits that are covered apart); tests/test_search_limit_scenes.py shows on the CPU that each case reaches the key,
the loop or the launch it is there for.  Every output is compared as bytes with the sequential models (tests/fuse_model.py,
tests/linefuse_model.py, tests/mappoint_model.py, tests/triangulate_model.py), the slots beyond the counts included, in the device-memory
form with canaries around every array, inputs included, and once per entry in the host-memory form at its largest case; the debug
accessors of the two fusions and of the triangulation are compared on the items that searched."""
import numpy as np
import pytest

from tests import search_limit_scenes as S
from tests.cull_scenes import DevArray, device_filled, host_filled

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher():
    from manhattanslam_amd.match import Matcher
    h = Matcher()
    yield h
    h.close()


def differing(got, want):
    """The outputs whose bytes differ from the expectation, each with the first places."""
    bad = []
    for k, w in want.items():
        g = got[k]
        if g.shape != w.shape or g.dtype != w.dtype:
            bad.append((k, g.shape, w.shape, g.dtype, w.dtype))
        elif g.tobytes() != w.tobytes():
            gb, wb = (np.ascontiguousarray(x).view(np.uint8).reshape(x.shape + (x.dtype.itemsize,)) for x in (g, w))
            at = np.argwhere((gb != wb).any(-1))
            bad.append((k, len(at), [(tuple(i), g[tuple(i)], w[tuple(i)]) for i in at[:6]]))
    return bad


def run(handle, form, call, a, out_shapes, inout=None):
    """One entry in the device-memory or the host-memory form: call(ins, outs, mem) with the inputs `a`, outputs that hold FILL
    (out_shapes: name -> (shape, dtype)) and arrays read and written in place (inout: name -> initial content).  Returns the outputs as
    numpy arrays; in device memory every canary of every array is checked."""
    dev = form == "device"
    ins = {k: (DevArray(v) if dev else v) for k, v in a.items()}
    outs = {k: (device_filled if dev else host_filled)(*v) for k, v in out_shapes.items()}
    for k, v in (inout or {}).items():
        outs[k] = DevArray(v) if dev else v.copy()
    call(ins, outs, int(dev))
    handle.sync()
    if dev:
        assert [k for k, v in list(ins.items()) + list(outs.items()) if not v.intact()] == []
        for k, v in ins.items():
            assert v.numpy().tobytes() == np.ascontiguousarray(a[k]).tobytes(), k      # inputs are left as they were
    return {k: (v.numpy() if dev else v) for k, v in outs.items()}


# ---- msl_fuse_candidates ---------------------------------------------------------------------------------------------------------------
def candidates(handle, case, forms=("device",)):
    from manhattanslam_amd._lib import check, lib, ptr
    a, sh, e = case["a"], case["sh"], case["e"]

    def call(i, o, mem):
        check(lib.msl_fuse_candidates(handle.h, sh["n_tab"], sh["cap"], sh["n_pts"], sh["n_items"], sh["tcap"], sh["lcap"], ptr(i["held_id"]),
                                      ptr(i["n_kps"]), ptr(i["pt_flags"]), ptr(i["targets"]), ptr(i["n_targets"]), mem, ptr(o["cand"]),
                                      ptr(o["n_cand"]), mem), "msl_fuse_candidates")
    for form in forms:
        got = run(handle, form, call, a, dict(cand=((sh["n_items"], sh["lcap"]), np.int32), n_cand=((sh["n_items"],), np.int32)))
        assert differing(got, e) == [], form


def test_c1_64_targets_of_8192_slots_into_lcap_65536(matcher):
    c = S.c1()
    assert c["e"]["n_cand"].tolist()[1] == S.MAX_LCAP - 1 and c["e"]["n_cand"][0] > S.MAX_LCAP
    candidates(matcher, c, forms=("device", "host"))


def test_c2_a_million_points_in_launches_of_16_16_and_8_items(matcher):
    c = S.c2()
    assert c["sh"]["n_pts"] == S.MAX_PTS and c["sh"]["n_items"] == 40
    candidates(matcher, c)


def test_c3_4096_items_in_one_launch(matcher):
    c = S.c3()
    assert c["sh"]["n_items"] == S.MAX_ITEMS
    candidates(matcher, c)


# ---- msl_covisibility ------------------------------------------------------------------------------------------------------------------
def covisibility(handle, case, forms=("device",)):
    from manhattanslam_amd._lib import check, lib, ptr
    a, sh, e = case["a"], case["sh"], case["e"]
    F, n_tab, ccap = sh["n_items"], sh["n_tab"], sh["ccap"]

    def call(i, o, mem):
        check(lib.msl_covisibility(handle.h, n_tab, sh["cap"], sh["n_pts"], F, sh["n_obs_total"], ccap, sh["th"], ptr(i["held_id"]), ptr(i["n_kps"]),
                                   ptr(i["pt_flags"]), ptr(i["obs_off"]), ptr(i["obs_kf"]), ptr(i["kf"]), mem, ptr(o["weight"]), ptr(o["conn"]),
                                   ptr(o["conn_w"]), ptr(o["n_conn"]), mem), "msl_covisibility")
    shapes = dict(weight=((F, n_tab), np.int32), conn=((F, ccap), np.int32), conn_w=((F, ccap), np.int32), n_conn=((F,), np.int32))
    for form in forms:
        got = run(handle, form, call, a, shapes)
        assert differing(got, e) == [], form


def test_v1_weight_8192_and_4095_connections(matcher):
    c = S.v1()
    assert c["e"]["n_conn"].tolist() == [S.MAX_TAB - 1] and c["e"]["conn_w"][0, 0] == S.MAX_CAP
    covisibility(matcher, c, forms=("device", "host"))


def test_v2_every_keyframe_of_4096_is_an_item(matcher):
    c = S.v2()
    assert c["e"]["weight"].shape == (S.MAX_TAB, S.MAX_TAB)
    covisibility(matcher, c)


# ---- msl_refresh_map_points ------------------------------------------------------------------------------------------------------------
def refresh(handle, case, forms=("device",)):
    from manhattanslam_amd import mappoint
    from manhattanslam_amd._lib import check, lib, ptr
    a, sh, e = case["a"], case["sh"], case["e"]
    prm = mappoint.refresh_params(case["facts"]["prm"]["scale_factors"])
    F = sh["n_items"]

    def call(i, o, mem):
        check(lib.msl_refresh_map_points(handle.h, sh["n_tab"], sh["cap"], sh["n_pts"], F, sh["n_obs_total"], sh["what"], ptr(prm),
                                         *[ptr(i[k]) for k in mappoint.TABLE_KEYS], *[ptr(i[k]) for k in mappoint.OBS_KEYS],
                                         *[ptr(i[k]) for k in mappoint.POINT_KEYS], ptr(i["ids"]), mem, *[ptr(o[k]) for k in mappoint.OUT_KEYS],
                                         *[ptr(o[k]) for k in mappoint.ROW_KEYS], mem), "msl_refresh_map_points")
    shapes = {k: (v.shape, v.dtype) for k, v in mappoint.refresh_outputs(1).items()}
    shapes = {k: ((F,) + s[1:], d) for k, (s, d) in shapes.items()}
    rows = dict(pt_desc=S.filled((sh["n_pts"], 32), np.uint8), pt_normal=S.filled((sh["n_pts"], 3), np.float32),
                pt_dist=S.filled((sh["n_pts"], 2), np.float32))
    for form in forms:
        got = run(handle, form, call, a, shapes, inout=rows)
        assert differing(got, e) == [], form                                # the rows not named keep their sentinel bytes


def test_r1_a_million_points_over_4096_keyframes(matcher):
    c = S.r1()
    assert (c["sh"]["n_pts"], c["sh"]["n_tab"]) == (S.MAX_PTS, S.MAX_TAB)
    refresh(matcher, c)


def test_r1c_a_million_points_over_keyframes_of_8192_keypoints(matcher):
    c = S.r1c()
    assert (c["sh"]["n_pts"], c["sh"]["cap"]) == (S.MAX_PTS, S.MAX_CAP)
    refresh(matcher, c)


def test_r2_every_point_of_a_million_is_an_item(matcher):
    c = S.r2()
    assert c["sh"]["n_items"] == c["sh"]["n_pts"] == S.MAX_PTS
    refresh(matcher, c, forms=("device", "host"))


# ---- msl_fuse_map_points ---------------------------------------------------------------------------------------------------------------
def fuse_points(handle, case, forms=("device",), debug=()):
    """debug: (item, model result) pairs whose msl_debug_fuse arrays are compared after the device-memory call."""
    from manhattanslam_amd import fuse
    from manhattanslam_amd._lib import check, lib, ptr
    from tests.test_fuse_gpu import _params
    a, sh, e = case["a"], case["sh"], case["e"]
    prm = _params(case["prm"])
    F, lcap = sh["n_items"], sh["lcap"]

    def call(i, o, mem):
        check(lib.msl_fuse_map_points(handle.h, sh["n_tab"], sh["cap"], sh["n_pts"], F, sh["n_lists"], lcap, ptr(prm), *[ptr(i[k]) for k in fuse.TABLE_KEYS],
                                      *[ptr(i[k]) for k in fuse.POINT_KEYS], ptr(i["tgt"]), ptr(i["list"]), ptr(i["cand"]), ptr(i["n_cand"]), mem,
                                      *[ptr(o[k]) for k in fuse.OUT_KEYS], mem), "msl_fuse_map_points")
    shapes = {k: (v.shape, v.dtype) for k, v in fuse.outputs(F, lcap).items()}
    for form in forms:
        got = run(handle, form, call, a, shapes)
        assert differing(got, e) == [], form
        if form == "device":
            for f, res in debug:
                assert differing(fuse.debug_fuse(handle, f, lcap), S.debug_arrays(res, lcap)) == [], f


def test_p1_a_keyframe_of_8192_keypoints_and_a_list_of_65536(matcher):
    c = S.p1()
    assert (c["sh"]["cap"], c["sh"]["lcap"], c["sh"]["n_pts"]) == (S.MAX_CAP, S.MAX_LCAP, S.MAX_PTS) and len(c["lst"]) == S.MAX_LCAP
    fuse_points(matcher, c, forms=("device", "host"), debug=[(0, c["res"][0])])


def test_p2_4096_items_over_4096_keyframes_and_4096_lists(matcher):
    c = S.p2()
    assert (c["sh"]["n_items"], c["sh"]["n_tab"], c["sh"]["n_lists"]) == (S.MAX_ITEMS,) * 3
    res = c["res"]
    fuse_points(matcher, c, debug=[(0, res[0]), (5, res[S.PERIOD]), (S.MAX_ITEMS - 1, res[(S.MAX_ITEMS - 1) % S.PERIOD])])


# ---- msl_fuse_map_lines ----------------------------------------------------------------------------------------------------------------
def fuse_lines(handle, case, forms=("device",), debug=()):
    from manhattanslam_amd import linefuse
    from manhattanslam_amd._lib import check, lib, ptr
    a, sh, e, p = case["a"], case["sh"], case["e"], case["prm"]
    prm = linefuse.line_fuse_params(p["fx"], p["fy"], p["cx"], p["cy"], p["minX"], p["maxX"], p["minY"], p["maxY"], p["scale_factors"],
                                    p["log_scale_factor"], th=p["th"], th_low=p["th_low"])
    F, lcap = sh["n_items"], sh["lcap"]

    def call(i, o, mem):
        check(lib.msl_fuse_map_lines(handle.h, sh["n_tab"], sh["klcap"], sh["n_lines"], F, sh["n_lists"], lcap, ptr(prm),
                                     *[ptr(i[k]) for k in linefuse.TABLE_KEYS], *[ptr(i[k]) for k in linefuse.LINE_KEYS], ptr(i["tgt"]), ptr(i["list"]),
                                     ptr(i["cand"]), ptr(i["n_cand"]), mem, *[ptr(o[k]) for k in linefuse.OUT_KEYS], mem), "msl_fuse_map_lines")
    shapes = {k: (v.shape, v.dtype) for k, v in linefuse.outputs(F, lcap).items()}
    for form in forms:
        got = run(handle, form, call, a, shapes)
        assert differing(got, e) == [], form
        if form == "device":
            for f, res in debug:
                assert differing(linefuse.debug_line_fuse(handle, f, lcap), S.line_debug_arrays(res, lcap)) == [], f


def test_l1_a_keyframe_of_256_keylines_and_a_list_of_65536(matcher):
    c = S.l1()
    assert (c["sh"]["klcap"], c["sh"]["lcap"], c["sh"]["n_lines"]) == (S.MAX_KLCAP, S.MAX_LCAP, S.MAX_PTS) and len(c["lst"]) == S.MAX_LCAP
    fuse_lines(matcher, c, forms=("device", "host"), debug=[(0, c["res"][0])])


def test_l2_4096_items_over_4096_keyframes_and_4096_lists(matcher):
    c = S.l2()
    assert (c["sh"]["n_items"], c["sh"]["n_tab"], c["sh"]["n_lists"]) == (S.MAX_ITEMS,) * 3
    res = c["res"]
    fuse_lines(matcher, c, debug=[(0, res[0]), (5, res[S.PERIOD]), (S.MAX_ITEMS - 1, res[(S.MAX_ITEMS - 1) % S.PERIOD])])


# ---- msl_refresh_map_lines -------------------------------------------------------------------------------------------------------------
def test_r3_a_million_lines_over_4096_keyframes_of_256_keylines(matcher):
    from manhattanslam_amd import linefuse, mappoint
    from manhattanslam_amd._lib import check, lib, ptr
    c = S.r3()
    a, sh, e = c["a"], c["sh"], c["e"]
    assert (sh["n_lines"], sh["klcap"], sh["n_tab"]) == (S.MAX_PTS, S.MAX_KLCAP, S.MAX_TAB)
    prm = mappoint.refresh_params(c["facts"]["prm"]["scale_factors"])
    F = sh["n_items"]

    def call(i, o, mem):
        check(lib.msl_refresh_map_lines(matcher.h, sh["n_tab"], sh["klcap"], sh["n_lines"], F, sh["n_obs_total"], ptr(prm),
                                        *[ptr(i[k]) for k in linefuse.REFRESH_TABLE_KEYS], *[ptr(i[k]) for k in linefuse.OBS_KEYS],
                                        *[ptr(i[k]) for k in linefuse.REFRESH_LINE_KEYS], ptr(i["ids"]), mem,
                                        *[ptr(o[k]) for k in linefuse.REFRESH_OUT_KEYS], *[ptr(o[k]) for k in linefuse.ROW_KEYS], mem),
              "msl_refresh_map_lines")
    shapes = {k: (v.shape, v.dtype) for k, v in linefuse.refresh_outputs(F).items()}
    rows = dict(ln_normal=S.filled((sh["n_lines"], 3), np.float64), ln_dist=S.filled((sh["n_lines"], 2), np.float32))
    for form in ("device", "host"):
        got = run(matcher, form, call, a, shapes, inout=rows)
        assert differing(got, e) == [], form                                # the rows not named keep their sentinel bytes


# ---- msl_triangulate_new_points --------------------------------------------------------------------------------------------------------
def triangulation(handle, case, forms=("device",), debug=()):
    """debug: the items whose msl_debug_triangulate arrays are compared after the device-memory call, (item, index of its model result)."""
    from manhattanslam_amd import triangulate
    from manhattanslam_amd._lib import check, lib, ptr
    from tests.test_triangulate_gpu import _check_debug, _params
    a, sh, e = case["a"], case["sh"], case["e"]
    prm = _params(case["prm"])
    F, cap, ncap = sh["n_items"], sh["cap"], sh["ncap"]

    def call(i, o, mem):
        check(lib.msl_triangulate_new_points(handle.h, sh["n_tab"], cap, F, ncap, ptr(prm), *[ptr(i[k]) for k in triangulate.TABLE_KEYS], ptr(i["cur"]),
                                             ptr(i["neigh"]), ptr(i["n_neigh"]), mem, *[ptr(o[k]) for k in triangulate.OUT_KEYS], mem),
              "msl_triangulate_new_points")
    shapes = {k: (v.shape, v.dtype) for k, v in case["e"].items()}
    for form in forms:
        got = run(handle, form, call, a, shapes)
        assert differing(got, e) == [], form
        if form == "device":
            for f, q in debug:
                assert _check_debug(handle, f, case["res"][q], case["items"][q][1], cap) > 0, f


def test_t1_sixteen_neighbours_in_a_table_of_4096(matcher):
    c = S.t1()
    assert (c["sh"]["n_tab"], c["sh"]["ncap"]) == (S.MAX_TAB, 16) and c["items"][0][0] == S.MAX_TAB - 1
    triangulation(matcher, c, debug=[(0, 0)])


def test_t2_65535_items(matcher):
    c = S.t2()
    assert c["sh"]["n_items"] == 65535
    triangulation(matcher, c, forms=("device", "host"), debug=[(0, 0), (65534, 65534 % S.PERIOD)])

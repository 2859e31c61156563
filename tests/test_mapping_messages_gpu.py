"""The refusals of the LocalMapping entry points whose checks live in csrc/msl_mappoint_check.h, and of the two fusion debug readbacks, with
msl_last_error() compared in full: the `_batch` forms of msl_fuse_map_points, msl_fuse_map_lines, msl_triangulate_new_points and
msl_fuse_candidates on one item, one candidate, two keyframes of one feature; msl_debug_fuse and msl_debug_line_fuse on a handle that has
made no such call and on the item behind the last call's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TCW = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(np.float32)
SF = np.ones(1, np.float32)


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


def test_debug_readbacks_refuse_what_the_last_call_did_not_make():
    from manhattanslam_amd import fuse, linefuse
    from manhattanslam_amd.match import Matcher
    h = Matcher()
    try:
        for debug, run, scene, msg in (
                (fuse.debug_fuse, fuse.fuse_map_points, _points(), "msl_debug_fuse: invalid argument (item outside the last msl_fuse_map_points call?)"),
                (linefuse.debug_line_fuse, linefuse.fuse_map_lines, _lines(),
                 "msl_debug_line_fuse: invalid argument (item outside the last msl_fuse_map_lines call?)")):
            assert _refused(debug, h, 0, 1) == msg                     # no such call yet on this handle
            out = run(*scene, [(1, 0)], [[0]], handle=h)
            assert out["status"].shape == (1, 1)
            assert _refused(debug, h, 1, 1) == msg                     # the item behind the call's one item
            assert _refused(debug, h, -1, 1) == msg
            assert debug(h, 0, 1)["level"].shape == (1,)
    finally:
        h.close()

"""The refusals of the two fusion debug readbacks, with msl_last_error() compared in full: msl_debug_fuse and msl_debug_line_fuse on a handle
that has made no such call and on the item behind the last call's (one item, one candidate, two keyframes of one feature).  The refusals of
the entries themselves need no device and are in tests/test_mapping_abi.py."""
import pytest

from tests.test_mapping_abi import _lines, _points, _refused

pytestmark = pytest.mark.gpu


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

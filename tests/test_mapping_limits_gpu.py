"""msl_local_keyframes, msl_local_points, msl_local_lines, msl_cull_keyframes and msl_cull_recent on the GPU at the limits include/msl.h
accepts: n_tab 4096, cap 8192, ccap = n_tab, klcap = lcap 256, mcap = mlcap 32768, n_items 4096, n_pts 1 << 20 and 1 << 20 recent elements.
The scenes are those of tests/mapping_limit_scenes.py (cases a to k); tests/test_mapping_limit_scenes.py shows on the CPU that each reaches
the loop or layout it is there for.  Every output is compared as bytes with the sequential models of tests/localmap_model.py and
tests/cull_model.py, in the device-memory form with canaries around every array, and once per entry in the host-memory form at its largest
case.  Two pairs of limits are covered separately and not together: the top list position (e) and the top slot (d) of the stamp key, and
n_tab (i) and cap (j) of the culling, whose keypoint table would otherwise have 4096 x 8192 rows."""
import numpy as np
import pytest

from tests import cull_scenes as cs
from tests import localmap_scenes as ls
from tests import mapping_limit_scenes as ms

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher():
    from manhattanslam_amd.match import Matcher
    h = Matcher()
    yield h
    h.close()


def localmap(matcher, a, sh, e, mcap, mlcap, device=True):
    """The three entries on packed arrays: every output equals e, and in device memory every canary is intact."""
    keep = {}
    got = ls.run(a, sh, mcap, mlcap, mem=int(device), handle=matcher, keep=keep)
    assert ls.same(got, e) == []
    if device:
        assert [k for k, v in keep.items() if v is not None and not v.intact()] == []


def localmap_case(matcher, name, mcap, mlcap=2, forms=("device",), a=None):
    s, (packed, sh), want = ms.case(name)[0], ms.packed(name), ms.want(name)
    e = ls.expected(s, packed, sh, mcap, mlcap, want)
    for form in forms:
        localmap(matcher, packed if a is None or form == "host" else a, sh, e, mcap, mlcap, device=form == "device")


def culling(matcher, name, forms=("device",)):
    (a, sh), want = ms.packed(name), ms.want(name)
    e = cs.expected(sh, want)
    for form in forms:
        keep = {}
        got = cs.run(a, sh, mem=int(form == "device"), handle=matcher, keep=keep)
        assert cs.same(got, e) == [], form
        if form == "device":
            assert [k for k, v in keep.items() if not v.intact()] == []


# ---- msl_local_keyframes -----------------------------------------------------------------------------------------------------------------
def test_a_every_keyframe_of_4096_voted(matcher):
    want = ms.want("a")
    assert [len(w["kf"]["local_kf"]) for w in want] == [4096] * 3
    localmap_case(matcher, "a", mcap=8)


def test_b_walk_over_a_table_of_4096_with_ccap_4096(matcher):
    assert ms.packed("b")[1]["ccap"] == 4096 and ms.want("b")[1]["kf"]["local_kf"].count(4095) == 1
    localmap_case(matcher, "b", mcap=128, forms=("device", "host"))


def test_c_frames_of_8192_1025_and_1024_slots(matcher):
    assert ms.packed("c")[1]["cap"] == 8192
    localmap_case(matcher, "c", mcap=1024)


# ---- msl_local_points / msl_local_lines ---------------------------------------------------------------------------------------------------
def test_d_a_keyframe_of_8192_slots_with_mcap_32768(matcher):
    a, sh = ms.packed("d")
    assert sh["cap"] == 8192
    localmap_case(matcher, "d", mcap=ms.MAX_MCAP, forms=("device", "host"), a=ms.absent_ids(a, sh))


@pytest.mark.parametrize("off", [-1, 0, 1])
def test_d_output_capacity_ends_inside_a_later_chunk(matcher, off):
    a, sh = ms.packed("d")
    cut = ms.mcap_cut() + off
    assert cut < len(ms.want("d")[0]["points"]["local"])                   # n_local stays the full count
    localmap_case(matcher, "d", mcap=cut, a=ms.absent_ids(a, sh))


def test_e_a_list_of_4096_with_an_absent_and_a_repeated_keyframe(matcher):
    s, facts = ms.case("e")
    (a, sh), want = ms.packed("e"), ms.want("e")
    mcap = len(want[0]["points"]["local"]) + 2
    e = ls.expected(s, a, sh, mcap, 2, want)
    a = dict(a, prev_kf=a["prev_kf"].copy())
    a["prev_kf"][0, facts["absent_pos"]] = sh["n_tab"]                     # copied as it stands; msl_local_points finds no such keyframe
    e["local_kf"][0, facts["absent_pos"]] = sh["n_tab"]
    assert a["n_prev"][0] == 4096
    localmap(matcher, a, sh, e, mcap, 2)


@pytest.mark.parametrize("name", ["f", "f1"])
def test_f_n_local_at_mcap_32768_and_one_above(matcher, name):
    assert len(ms.want(name)[0]["points"]["local"]) == ms.MAX_MCAP + (name == "f1")
    localmap_case(matcher, name, mcap=ms.MAX_MCAP)


def test_g_line_rows_of_256_with_mlcap_32768(matcher):
    s, (a, sh), want = ms.case("g")[0], ms.packed("g"), ms.want("g")
    assert sh["klcap"] == sh["lcap"] == 256
    a = ms.line_payloads(dict(a, ln_xyz=a["ln_xyz"].copy(), ln_normal=a["ln_normal"].copy()), want[0]["lines"]["local"])
    e = ls.expected(s, a, sh, 4, ms.MAX_MCAP, want)
    n = int(e["n_local_lines"][0])
    words = e["ml_xyz"][0, :n].view(np.uint64)
    assert n > 256 and all((words == w).any() for w in ms.NAN_WORDS)       # copied by words: the payloads are in the expectation
    for device in (True, False):
        localmap(matcher, a, sh, e, 4, ms.MAX_MCAP, device=device)


def test_h_a_point_table_of_a_million_one_frame_of_stamps_at_a_time(matcher):
    from manhattanslam_amd import localmap as lmap
    s, (a, sh), want = ms.case("h")[0], ms.packed("h"), ms.want("h")
    a, sh, e = ms.pad_points(a, sh, ls.expected(s, a, sh, 256, 16, want))
    assert sh["n_pts"] == 1 << 20 and sh["n_frames"] == 3
    lmap.set_budget(matcher, 4 * sh["n_pts"])                              # one frame of stamps: three groups at the largest stamp row
    try:
        localmap(matcher, a, sh, e, 256, 16)
    finally:
        lmap.set_budget(matcher)


# ---- msl_cull_keyframes -------------------------------------------------------------------------------------------------------------------
def test_i_4096_items_one_of_them_over_all_4096_candidates(matcher):
    sh = ms.packed("i")[1]
    assert (sh["n_tab"], sh["ccap"], sh["n_items"]) == (4096, 4096, 4096)
    culling(matcher, "i", forms=("device", "host"))


def test_j_keyframes_of_8192_slots_on_either_side_of_nine_tenths(matcher):
    assert ms.packed("j")[1]["cap"] == 8192 and ms.want("j")[0][0] == ms.case("j")[1]["rows"]
    culling(matcher, "j")


# ---- msl_cull_recent ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("th_obs", [3, 2])
def test_k_a_million_recent_elements(matcher, form, th_obs):
    from manhattanslam_amd import cull
    from tests.test_cull_gpu import CUR
    n = ms.MAX_RECENT
    a, want = ms.recent_tiled(n, th_obs, form)
    d = {k: cs.DevArray(v) for k, v in a.items()}
    for m in (n, n - 255):                                                 # 4096 full blocks; 4095 and a block of one thread
        v = cull.cull_recent_device(matcher, m, CUR, th_obs, form, d, cs.device_filled((n,), np.uint8))
        matcher.sync()
        got = v.numpy()
        assert np.array_equal(got[:m], want[:m]) and (got[m:] == cs.FILL).all() and v.intact()
    assert all(x.intact() for x in d.values())
    h, hw = ms.recent_tiled(n, th_obs, form, host=True)
    assert np.array_equal(cull.cull_recent(n, CUR, th_obs, form, h, cs.host_filled((n,), np.uint8), handle=matcher), hw)

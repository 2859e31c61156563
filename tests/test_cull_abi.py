"""msl_cull_keyframes and msl_cull_recent are part of the C ABI: exported by libmsl.so, declared in include/msl.h and bound in _lib; the two
forms differ in their first argument only.  Their refusals, through the device-indexed forms on host memory, which check before they touch
a device: every limit, every NULL and every index defect of a host-memory call is refused with the field named, and the outputs keep
their bytes.  No launch (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import abi_refusals
from tests import cull_scenes as cs
from tests.abi_refusals import put

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"msl_cull_keyframes": 28, "msl_cull_recent": 13}


def test_exported_declared_and_bound():
    from manhattanslam_amd import _header, _lib
    dll = C.CDLL(_lib.LIB_PATH)
    src = _header.text("msl.h")
    decl = _header.declarations(src)
    for base, count in NAMES.items():
        for n in (base, base + "_batch"):
            assert decl[n][0] == "int" and hasattr(dll, n), n
            res, args = _lib.SIGNATURES[n]
            assert res is C.c_int and len(args) == len(decl[n][1]) == count, n
            assert getattr(_lib.lib, n).argtypes == args
        a, b = decl[base][1], decl[base + "_batch"][1]
        assert a[0] == ("msl_match *", "h") and b[0] == ("int", "device") and a[1:] == b[1:]
    assert _lib.RECORDS["msl_cull_params"].names == ("th_depth",) and _lib.RECORDS["msl_cull_params"].itemsize == 4


def test_argument_order_and_codes_are_the_wrapper_s():
    import manhattanslam_amd as m
    from manhattanslam_amd import _header, cull
    from tests import cull_model as cm
    assert m.cull is cull and all(callable(getattr(cull, n)) for n in cull.__all__ if n[0].islower())
    src = _header.text("msl.h")
    decl = _header.declarations(src)
    names = [x[1] for x in decl["msl_cull_keyframes"][1]]
    assert names[1:9] == ["n_tab", "cap", "n_pts", "n_items", "n_obs_total", "ccap", "origin", "params"] and tuple(names[9:22]) == cull.KF_IN_KEYS
    assert names[22] == "mem" and tuple(names[23:27]) == cull.KF_OUT_KEYS and names[27] == "out_mem"
    names = [x[1] for x in decl["msl_cull_recent"][1]]
    assert names[1:5] == ["n", "cur_kf_id", "th_obs", "ratio_form"] and tuple(names[5:10]) == cull.RECENT_IN_KEYS
    assert names[10:] == ["mem", "verdict", "out_mem"]
    define = lambda n: int(re.search(r"#define\s+%s\s+(\d+)\b" % n, src).group(1))
    for mod in (cull, cm):
        assert [define("MSL_CULL_" + n) for n in ("KEPT", "CULLED", "ORIGIN", "NOT_ERASE", "ABSENT")] == [mod.KEPT, mod.CULLED, mod.ORIGIN, mod.NOT_ERASE, mod.ABSENT]
        assert [define("MSL_RATIO_" + n) for n in ("FLOAT", "INT")] == [mod.RATIO_FLOAT, mod.RATIO_INT]
        assert [define("MSL_RECENT_" + n) for n in ("KEEP", "ERASE_BAD", "CULL_RATIO", "CULL_OBS", "RETIRE", "INVALID")] == \
            [mod.RECENT_KEEP, mod.RECENT_ERASE_BAD, mod.RECENT_CULL_RATIO, mod.RECENT_CULL_OBS, mod.RECENT_RETIRE, mod.RECENT_INVALID]
    # the tables are, name for name and type for type, those of the other LocalMapping entries; cand / n_cand are msl_covisibility's rows
    mine = {n: t for t, n in decl["msl_cull_keyframes"][1]}
    for entry, shared in (("msl_fuse_map_points", ("kps_un", "uright", "held_id", "n_kps", "pt_flags", "pt_nobs")),
                          ("msl_refresh_map_points", ("kf_flags", "obs_off", "obs_kf", "obs_idx")), ("msl_triangulate_new_points", ("depth",))):
        theirs = {n: t for t, n in decl[entry][1]}
        assert all(mine[k] == theirs[k] for k in shared), entry
    covis = {n: t for t, n in decl["msl_covisibility"][1]}
    assert mine["cand"] == "const " + covis["conn"] and mine["n_cand"] == "const " + covis["n_conn"]


def test_limits_are_the_header_s():
    from manhattanslam_amd import cull
    text = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", "msl.h")).read())
    line = re.search(r"Cull limits: n_tab <= (\d+), cap <= (\d+), n_pts <= (\d+), 1 <= n_items <= (\d+), n_obs_total >= 0, 1 <= ccap <= n_tab; "
                     r"1 <= n <= (\d+), cur_kf_id >= 0, th_obs >= 0", text)
    assert tuple(int(x) for x in line.groups()) == (cull.MAX_TAB, cull.MAX_CAP, cull.MAX_PTS, cull.MAX_ITEMS, cull.MAX_RECENT)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    from manhattanslam_amd import cull
    s = cs.random_scene(4, 6, 5, n_items=2)
    s["items"], s["origin"] = [[2, 0, 5], [1, 3]], 4
    a, sh = cs.pack(s, cap=5, ccap=4)
    a["params"] = cull.cull_params(sh["th_depth"])
    n = 7
    a.update(found=np.arange(n, dtype=np.int32), visible=np.arange(1, n + 1, dtype=np.int32), first_kf_id=np.full(n, 3, np.int32),
             nobs=np.full(n, 4, np.int32), flags=np.ones(n, np.uint8))
    return a, dict(sh, n=n, cur_kf_id=5, th_obs=3, ratio_form=1)


def refused(entry, scene, **over):
    from manhattanslam_amd import cull
    a, sh = scene
    out = dict(cull.keyframes_outputs(sh["n_items"], sh["ccap"], cs.host_filled), verdict=cs.host_filled((sh["n"],), np.uint8))
    return abi_refusals.refused(entry, sh, a, out, **over)


LIMITS = {"msl_cull_keyframes": [("n_tab", 0, "n_tab 0 outside 1 .. 4096"), ("n_tab", 4097, "n_tab 4097 outside 1 .. 4096"),
                                 ("cap", 0, "cap 0 outside 1 .. 8192"), ("cap", 8193, "cap 8193 outside 1 .. 8192"),
                                 ("n_pts", 0, "n_pts 0 outside 1 .. 1048576"), ("n_pts", (1 << 20) + 1, "n_pts 1048577 outside 1 .. 1048576"),
                                 ("n_items", 0, "n_items 0 outside 1 .. 4096"), ("n_items", 4097, "n_items 4097 outside 1 .. 4096"),
                                 ("n_obs_total", -1, "n_obs_total -1 below 0"), ("ccap", 0, "ccap 0 outside 1 .. n_tab = 6"),
                                 ("ccap", 7, "ccap 7 outside 1 .. n_tab = 6"), ("origin", 6, "origin is keyframe 6 of 6"),
                                 ("origin", -2, "origin is keyframe -2 of 6")],
          "msl_cull_recent": [("n", 0, "n 0 outside 1 .. 1048576"), ("n", (1 << 20) + 1, "n 1048577 outside 1 .. 1048576"),
                              ("cur_kf_id", -1, "cur_kf_id -1 below 0"), ("th_obs", -1, "th_obs -1 below 0"),
                              ("ratio_form", 2, "ratio_form 2 is neither MSL_RATIO_FLOAT nor MSL_RATIO_INT"),
                              ("ratio_form", -1, "ratio_form -1 is neither MSL_RATIO_FLOAT nor MSL_RATIO_INT")]}


@pytest.mark.parametrize("entry", sorted(NAMES))
def test_every_limit_is_refused_with_the_field_named(scene, entry):
    from manhattanslam_amd import _header
    assert {l[0] for l in LIMITS[entry]} == {n for t, n in _header.declarations(_header.text("msl.h"))[entry][1][1:] if t == "int"}
    for field, value, msg in LIMITS[entry]:
        assert refused(entry, scene, **{field: value}) == f"{entry}: {msg}"


@pytest.mark.parametrize("entry", sorted(NAMES))
def test_every_null_is_refused_with_the_field_named(scene, entry):
    from manhattanslam_amd import _header
    pointers = [n for t, n in _header.declarations(_header.text("msl.h"))[entry][1][1:] if t.endswith("*")]
    assert len(pointers) == {"msl_cull_keyframes": 18, "msl_cull_recent": 6}[entry]
    for n in pointers:
        assert refused(entry, scene, **{n: None}) == f"{entry}: {n} is NULL"


def test_index_defects_of_a_host_memory_call_are_refused(scene):
    kf, rc = "msl_cull_keyframes", "msl_cull_recent"
    assert refused(kf, scene, cand=put((0, 1), 6)) == f"{kf}: cand[0][1] is keyframe 6 of 6"
    assert refused(kf, scene, cand=put((1, 0), -1)) == f"{kf}: cand[1][0] is keyframe -1 of 6"
    assert refused(kf, scene, cand=put((0, 2), 2)) == f"{kf}: cand[0] holds keyframe 2 twice"
    assert refused(kf, scene, n_cand=put(1, 5)) == f"{kf}: n_cand[1] is 5 outside 0 .. ccap = 4"
    assert refused(kf, scene, n_cand=put(0, -1)) == f"{kf}: n_cand[0] is -1 outside 0 .. ccap = 4"
    assert refused(kf, scene, obs_kf=put(0, 6)) == f"{kf}: obs_kf[0] is keyframe 6 of 6"
    assert refused(kf, scene, obs_idx=put(0, 5)).startswith(f"{kf}: obs_idx[0] is keypoint 5 of ")
    assert refused(kf, scene, obs_idx=put(0, -1)).startswith(f"{kf}: obs_idx[0] is keypoint -1 of ")
    assert refused(kf, scene, obs_off=put(3, 1000)).startswith(f"{kf}: obs_off descends at point 3")
    assert refused(rc, scene, found=put(2, -1)) == f"{rc}: found[2] is -1, below 0"
    assert refused(rc, scene, visible=put(6, -4)) == f"{rc}: visible[6] is -4, below 0"
    assert refused(rc, scene, first_kf_id=put(0, -1)) == f"{rc}: first_kf_id[0] is -1, below 0"
    assert refused(rc, scene, visible=put(4, 0)) == f"{rc}: visible[4] is 0 in the integer ratio form (a division by zero in the reference)"


def test_the_handle_forms_refuse_a_null_handle():
    from manhattanslam_amd import _lib
    for entry, count in NAMES.items():
        args = [0 if t in (C.c_int, C.c_uint) else None for t in _lib.SIGNATURES[entry][1][1:]]
        assert len(args) == count - 1 and getattr(_lib.lib, entry)(None, *args) == -1
        assert _lib.lib.msl_last_error().decode() == f"{entry}: h is NULL"

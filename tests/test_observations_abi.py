"""msl_observations_apply is part of the C ABI: exported by libmsl.so, declared in include/msl.h and bound in _lib; the two forms differ
in their first argument only; the arrays it shares with the other LocalMapping entries have their names and types.  Its refusals, through
the device-indexed form on host memory, which checks before it touches a device: every limit, every NULL and every index defect of a
host-memory call is refused with the field named, and the in-place arrays and the outputs keep their bytes.  No launch (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import abi_refusals
from tests import observations_model as om
from tests import observations_scenes as osc
from tests.abi_refusals import put

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY, COUNT = "msl_observations_apply", 29
OPTIONAL = ("uright", "pt_found", "pt_visible", "pt_replaced")


def test_exported_declared_and_bound():
    from manhattanslam_amd import _header, _lib
    dll = C.CDLL(_lib.LIB_PATH)
    decl = _header.declarations(_header.text("msl.h"))
    for n in (ENTRY, ENTRY + "_batch"):
        assert decl[n][0] == "int" and hasattr(dll, n), n
        res, args = _lib.SIGNATURES[n]
        assert res is C.c_int and len(args) == len(decl[n][1]) == COUNT, n
        assert getattr(_lib.lib, n).argtypes == args
    a, b = decl[ENTRY][1], decl[ENTRY + "_batch"][1]
    assert a[0] == ("msl_match *", "h") and b[0] == ("int", "device") and a[1:] == b[1:]
    assert _lib.RECORDS["msl_obs_op"].names == ("op", "a", "b", "c") and _lib.RECORDS["msl_obs_op"].itemsize == 16


def test_argument_order_codes_and_limits_are_the_wrapper_s():
    import manhattanslam_amd as m
    from manhattanslam_amd import _header, observations as ob
    assert m.observations is ob and all(callable(getattr(ob, n)) for n in ob.__all__ if n[0].islower())
    src = _header.text("msl.h")
    decl = _header.declarations(src)
    names = [x[1] for x in decl[ENTRY][1]]
    assert names[1:8] == ["n_tab", "cap", "n_pts", "n_obs_total", "n_ops", "ocap", "tcap"] and tuple(names[8:14]) == ob.IN_KEYS
    assert tuple(names[14:21]) == ob.INOUT_KEYS and names[21] == "mem" and tuple(names[22:28]) == ob.OUT_KEYS and names[28] == "out_mem"
    define = lambda n: int(re.search(r"#define\s+%s\s+(\d+)\b" % n, src).group(1))
    for mod in (ob, om):
        assert [define("MSL_OBS_" + n) for n in ("ADD", "ERASE", "SET_BAD", "REPLACE", "KF_ERASE")] == [mod.ADD, mod.ERASE, mod.SET_BAD, mod.REPLACE, mod.KF_ERASE]
        assert [define("MSL_OBS_" + n) for n in ("CHANGED", "TURNED_BAD")] == [mod.CHANGED, mod.TURNED_BAD]
        assert [define("MSL_OBS_" + n) for n in ("MAX", "MAX_OPS", "MAX_KF_ERASE")] == [mod.OBS_MAX, mod.MAX_OPS, mod.MAX_KF_ERASE]
    text = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", "msl.h")).read())
    line = re.search(r"Limits: n_tab <= (\d+), cap <= (\d+), n_pts <= (\d+), n_obs_total >= 0, 1 <= n_ops <= (\d+) of which at most (\d+) "
                     r"MSL_OBS_KF_ERASE, ocap >= n_obs_total \+ the number of MSL_OBS_ADD ops", text)
    assert tuple(int(x) for x in line.groups()) == (ob.MAX_TAB, ob.MAX_CAP, ob.MAX_PTS, ob.MAX_OPS, ob.MAX_KF_ERASE)


def test_shared_arrays_have_the_names_and_types_of_the_other_entries():
    from manhattanslam_amd import _header
    decl = _header.declarations(_header.text("msl.h"))
    mine = {n: t for t, n in decl[ENTRY][1]}
    cull = {n: t for t, n in decl["msl_cull_keyframes"][1]}
    refresh = {n: t for t, n in decl["msl_refresh_map_points"][1]}
    for k in ("n_kps", "uright", "obs_off", "obs_kf", "obs_idx"):
        assert mine[k] == cull[k], k
    for k in ("held_id", "pt_flags", "pt_nobs"):                           # in place here: the consumers' type without its const
        assert "const " + mine[k] == cull[k], k
    assert "const " + mine["pt_ref"] == refresh["pt_ref"] and refresh["obs_off"] == mine["obs_off"]
    for k in ("obs_off", "obs_kf", "obs_idx"):                             # the new table is the next call's table
        assert "const " + mine[k + "_out"] == mine[k], k
    assert mine["touched"] == refresh["ids"].replace("const ", "")         # ids = touched, n_items = tcap


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    s, ops = osc.pin_kf_erase()
    a, sh = osc.pack(s, ops)
    assert sh == dict(n_tab=4, cap=6, n_pts=5, n_obs_total=12, n_ops=4, ocap=13, tcap=5) and [o[0] for o in ops] == [om.KF_ERASE, om.KF_ERASE, om.ADD, om.ERASE]
    return a, sh


def op(o, field, value):
    """The edit ops[o].field = value."""
    def edit(x):
        x[field][o] = value
    return edit


def refused(scene, **over):
    from manhattanslam_amd import observations as ob
    a, sh = scene
    out = ob.outputs(sh["n_pts"], sh["n_ops"], sh["ocap"], sh["tcap"], osc.host_filled)
    return abi_refusals.refused(ENTRY, sh, a, out, inout=ob.INOUT_KEYS, **over)


LIMITS = [("n_tab", 0, "n_tab 0 outside 1 .. 4096"), ("n_tab", 4097, "n_tab 4097 outside 1 .. 4096"), ("cap", 0, "cap 0 outside 1 .. 8192"),
          ("cap", 8193, "cap 8193 outside 1 .. 8192"), ("n_pts", 0, "n_pts 0 outside 1 .. 1048576"),
          ("n_pts", (1 << 20) + 1, "n_pts 1048577 outside 1 .. 1048576"), ("n_obs_total", -1, "n_obs_total -1 below 0"),
          ("n_ops", 0, "n_ops 0 outside 1 .. 65536"), ("n_ops", 65537, "n_ops 65537 outside 1 .. 65536"),
          ("ocap", 11, "ocap 11 below n_obs_total = 12"), ("ocap", 12, "ocap is 12, below n_obs_total + the 1 MSL_OBS_ADD ops = 13"),
          ("tcap", 0, "tcap 0 outside 1 .. n_pts = 5"), ("tcap", 6, "tcap 6 outside 1 .. n_pts = 5")]


def test_every_limit_is_refused_with_the_field_named(scene):
    assert {l[0] for l in LIMITS} == set(abi_refusals.declared(ENTRY)[0])
    for field, value, msg in LIMITS:
        assert refused(scene, **{field: value}) == f"{ENTRY}: {msg}"


def test_every_null_but_the_optional_ones_is_refused_with_the_field_named(scene):
    pointers = abi_refusals.declared(ENTRY)[1]
    assert len(pointers) == 19 and set(OPTIONAL) < set(pointers)
    for n in pointers:
        if n not in OPTIONAL:
            assert refused(scene, **{n: None}) == f"{ENTRY}: {n} is NULL"
    assert refused(scene, pt_found=None) == f"{ENTRY}: pt_found is NULL while pt_visible is given"
    assert refused(scene, pt_visible=None) == f"{ENTRY}: pt_visible is NULL while pt_found is given"


def test_index_defects_of_a_host_memory_call_are_refused(scene):
    e = ENTRY
    assert refused(scene, obs_kf=put(0, 4)) == f"{e}: obs_kf[0] is keyframe 4 of 4"
    assert refused(scene, obs_idx=put(0, 6)).startswith(f"{e}: obs_idx[0] is keypoint 6 of ")
    assert refused(scene, obs_off=put(3, 1000)).startswith(f"{e}: obs_off descends at point 3")
    assert refused(scene, obs_kf=put(1, 0)) == f"{e}: obs_kf[1] is keyframe 0 after 0 in the range of point 0: not strictly ascending"
    assert refused(scene, obs_kf=put(2, 0)) == f"{e}: obs_kf[2] is keyframe 0 after 1 in the range of point 0: not strictly ascending"
    assert refused(scene, ops=op(0, "op", 0)) == f"{e}: ops[0].op is 0, not an MSL_OBS_* code"
    assert refused(scene, ops=op(3, "op", 6)) == f"{e}: ops[3].op is 6, not an MSL_OBS_* code"
    assert refused(scene, ops=op(2, "a", 5)) == f"{e}: ops[2].a is id 5 of 5"
    assert refused(scene, ops=op(3, "a", -1)) == f"{e}: ops[3].a is id -1 of 5"
    assert refused(scene, ops=op(1, "b", 4)) == f"{e}: ops[1].b is keyframe 4 of 4"
    assert refused(scene, ops=op(3, "b", -1)) == f"{e}: ops[3].b is keyframe -1 of 4"
    assert refused(scene, ops=op(2, "c", 6)) == f"{e}: ops[2].c is keypoint 6 of 6 in keyframe 3"
    assert refused(scene, ops=op(2, "c", -1)) == f"{e}: ops[2].c is keypoint -1 of 6 in keyframe 3"
    assert refused(scene, ops=op(3, "op", om.KF_ERASE)) == f"{e}: ops[3] is an MSL_OBS_KF_ERASE behind another op"

    def replace(x):
        x[3] = (om.REPLACE, 1, 5, 0)
    assert refused(scene, ops=replace) == f"{e}: ops[3].b is id 5 of 5"


def test_more_kf_erase_than_the_limit_is_refused(scene):
    from manhattanslam_amd import observations as ob
    a, sh = scene
    ops = ob.pack_ops([(om.KF_ERASE, 0, 1)] * 257)
    out = ob.outputs(sh["n_pts"], 257, sh["ocap"], sh["tcap"], osc.host_filled)
    msg = abi_refusals.refused(ENTRY, dict(sh, n_ops=257), dict(a, ops=ops), out, inout=ob.INOUT_KEYS)
    assert msg == f"{ENTRY}: ops[256] is MSL_OBS_KF_ERASE number 257 of at most 256"


def test_the_handle_form_refuses_a_null_handle():
    from manhattanslam_amd import _lib
    args = [0 if t in (C.c_int, C.c_uint) else None for t in _lib.SIGNATURES[ENTRY][1][1:]]
    assert len(args) == COUNT - 1 and getattr(_lib.lib, ENTRY)(None, *args) == -1
    assert _lib.lib.msl_last_error().decode() == f"{ENTRY}: h is NULL"

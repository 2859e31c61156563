"""msl_points_3d and msl_keyframe_decision are part of the C ABI: exported by libmsl.so, declared in include/msl.h and bound in _lib; the two
forms differ in their first argument only; the records have the header's layout, the constants its values, the Python wrapper its names.
Their refusals, through the device-indexed forms on host memory, which check before they touch a device: every limit, every NULL and every
index defect of a host-memory call is refused with the field named, and the outputs keep their bytes.  No launch (no GPU needed)."""
import ctypes as C
import re

import numpy as np
import pytest

from tests import abi_refusals
from tests import keyframe_model as km
from tests import keyframe_scenes as ks
from tests.abi_refusals import put

NAMES = {"msl_points_3d": 27, "msl_keyframe_decision": 39}


def test_exported_declared_and_bound():
    from manhattanslam_amd import _header, _lib
    dll = C.CDLL(_lib.LIB_PATH)
    decl = _header.declarations(_header.text("msl.h"))
    for base, count in NAMES.items():
        for n in (base, base + "_batch"):
            assert decl[n][0] == "int" and hasattr(dll, n), n
            res, args = _lib.SIGNATURES[n]
            assert res is C.c_int and len(args) == len(decl[n][1]) == count, n
            assert getattr(_lib.lib, n).argtypes == args
        a, b = decl[base][1], decl[base + "_batch"][1]
        assert a[0] == ("msl_match *", "h") and b[0] == ("int", "device") and a[1:] == b[1:]


def test_record_layouts_are_the_header_s():
    from manhattanslam_amd import _lib, keyframe
    p = _lib.RECORDS["msl_point3d_params"]
    assert p.names == ("fx", "fy", "cx", "cy", "th_depth", "min_points", "nlevels", "scale_factors") and p.itemsize == 92
    assert [p.fields[n][1] for n in p.names] == [0, 4, 8, 12, 16, 20, 24, 28] and p.fields["scale_factors"][0].shape == (16,)
    r = _lib.RECORDS["msl_keyframe_frame"]
    assert r.names == ("flags", "frame_id", "last_keyframe_id", "last_reloc_frame_id", "n_kfs", "ref_kf", "n_inliers_in", "local_mapping_idle",
                       "local_mapping_stopped", "keyframes_in_queue") == keyframe.FRAME_FIELDS
    assert r.itemsize == 40 and all(r.fields[n] == (np.dtype("<i4"), 4 * i) for i, n in enumerate(r.names))
    q = _lib.RECORDS["msl_keyframe_params"]
    assert q.names == ("max_frames", "min_frames", "th_depth", "only_tracking") and q.itemsize == 16 and q.fields["th_depth"][0] == np.dtype("<f4")
    assert keyframe.POINT3D_PARAMS_DTYPE is p and keyframe.KEYFRAME_FRAME_DTYPE is r and keyframe.KEYFRAME_PARAMS_DTYPE is q
    assert set(ks.RECORD) == set(r.names)


def test_argument_order_and_constants_are_the_wrapper_s():
    import manhattanslam_amd as m
    from manhattanslam_amd import _header, keyframe
    assert m.keyframe is keyframe and all(callable(getattr(keyframe, n)) for n in keyframe.__all__ if n[0].islower())
    src = _header.text("msl.h")
    decl = _header.declarations(src)
    names = [x[1] for x in decl["msl_points_3d"][1]]
    assert names[1:6] == ["n_frames", "cap", "n_pts", "mode", "params"] and tuple(names[6:15]) == keyframe.POINT_IN_KEYS
    assert names[15] == "mem" and tuple(names[16:26]) == keyframe.POINT_OUT_KEYS and names[26] == "out_mem"
    assert tuple(keyframe.points_outputs(1, 1)) == keyframe.POINT_OUT_KEYS
    names = [x[1] for x in decl["msl_keyframe_decision"][1]]
    assert names[1:9] == ["n_frames", "cap", "lcap", "pcap", "n_tab", "n_pts", "n_lines", "params"] and tuple(names[9:23]) == keyframe.DECISION_IN_KEYS
    assert names[23] == "mem" and tuple(names[24:26]) == keyframe.DECISION_INOUT_KEYS and tuple(names[26:38]) == keyframe.DECISION_OUT_KEYS
    assert names[38] == "out_mem" and tuple(keyframe.decision_outputs(1, 1, 1)) == keyframe.DECISION_OUT_KEYS
    define = lambda n: int(re.search(r"#define\s+%s\s+(\d+)\b" % n, src).group(1))
    for mod in (keyframe, km):
        assert [define("MSL_POINT3D_" + n) for n in ("ALL", "KEYFRAME", "FRAME")] == [mod.ALL, mod.KEYFRAME, mod.FRAME]
        assert [define("MSL_KF_" + n) for n in ("TRACKED_LOCAL_MAP", "TRACK_OK", "NEW_PLANE")] == [mod.TRACKED_LOCAL_MAP, mod.TRACK_OK, mod.NEW_PLANE]
        assert [define("MSL_KF_" + n) for n in ("C1A", "C1B", "C1C", "C2")] == [mod.C1A, mod.C1B, mod.C1C, mod.C2]
    # the tables and frame arrays are, name for name and type for type, those of the entries they chain with
    mine = {n: t for t, n in decl["msl_points_3d"][1]}
    theirs = {n: t for t, n in decl["msl_local_points"][1]}
    assert all(mine[k] == theirs[k] for k in ("cur_held", "pt_nobs"))
    for k, other in (("new_xyz", "mp_xyz"), ("new_normal", "mp_normal"), ("new_dist", "mp_dist"), ("new_desc", "mp_desc")):
        assert mine[k] == theirs[other]
    mine = {n: t for t, n in decl["msl_keyframe_decision"][1]}
    assert all(mine[k] == theirs[k] for k in ("cur_held", "n_cur", "pt_nobs", "pt_flags", "held_id", "n_kps"))
    plane = {n: t for t, n in decl["msl_plane_associate"][1]}
    pose = {n: t for t, n in decl["msl_pose_optimize"][1]}
    assert mine["plane_match"] == plane["plane_match"] and mine["plane_outlier"] == pose["plane_outlier"] and mine["outlier"] == "const " + pose["outlier"]


def test_limits_are_the_header_s():
    import os
    from manhattanslam_amd import keyframe
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(root, "include", "msl.h")).read())
    line = re.search(r"Limits: n_frames >= 1, cap <= (\d+), 0 <= n_pts <= (\d+), mode one of MSL_POINT3D_\*, 1 <= nlevels <= MSL_MATCH_MAX_LEVELS, min_points >= 0", text)
    assert tuple(int(x) for x in line.groups()) == (keyframe.MAX_CAP, keyframe.MAX_PTS)
    line = re.search(r"Limits: n_frames >= 1, cap <= (\d+), lcap <= (\d+), pcap <= (\d+), n_tab <= (\d+), n_pts <= (\d+), n_lines <= (\d+) \(each at least 1\)", text)
    assert tuple(int(x) for x in line.groups()) == (keyframe.MAX_CAP, keyframe.MAX_LCAP, keyframe.MAX_PCAP, keyframe.MAX_TAB, keyframe.MAX_PTS, keyframe.MAX_LINES)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    from manhattanslam_amd import keyframe
    t = ks.table()
    frames = [ks.point_frame(70, 5), ks.point_frame(71, 3)]
    cap, a = keyframe.pack_points(frames, cap=6)
    a.update(pt_nobs=t["pt_nobs"], enable=np.ones(2, np.int32), first_id=np.zeros(2, np.int32),
             params=keyframe.point3d_params(500.0, 500.0, 320.0, 240.0, 3.0, km.params()["scale_factors"]))
    dframes = [ks.decision_frame(70, 5, 2, 1), ks.decision_frame(71, 3, 4, 2)]
    _, lcap, pcap, d = keyframe.pack_decision(dframes, cap=6, lcap=4, pcap=2)
    held, n_kps = ks.table_arrays(6)
    d.update(pt_nobs=t["pt_nobs"], pt_flags=t["pt_flags"], ln_nobs=t["ln_nobs"], held_id=held, n_kps=n_kps, params=keyframe.keyframe_params(30, 0, 3.0))
    sh = dict(n_frames=2, cap=6, n_pts=ks.N_PTS, mode=km.KEYFRAME, lcap=4, pcap=2, n_tab=ks.N_TAB, n_lines=ks.N_LINES)
    return {"msl_points_3d": a, "msl_keyframe_decision": d}, sh


def refused(entry, scene, **over):
    from manhattanslam_amd import keyframe
    arrays, sh = scene
    out = keyframe.points_outputs(2, 6, ks.host_filled) if entry == "msl_points_3d" else keyframe.decision_outputs(2, 6, 4, ks.host_filled)
    return abi_refusals.refused(entry, sh, arrays[entry], out, inout=[k for k in keyframe.DECISION_INOUT_KEYS if k in arrays[entry]], **over)


LIMITS = {"msl_points_3d": [("n_frames", 0, "n_frames 0 below 1"), ("cap", 0, "cap 0 outside 1 .. 8192"), ("cap", 8193, "cap 8193 outside 1 .. 8192"),
                            ("n_pts", -1, "n_pts -1 outside 0 .. 1048576"), ("n_pts", (1 << 20) + 1, "n_pts 1048577 outside 0 .. 1048576"),
                            ("mode", 3, "mode 3 is not an MSL_POINT3D_* value"), ("mode", -1, "mode -1 is not an MSL_POINT3D_* value")],
          "msl_keyframe_decision": [("n_frames", 0, "n_frames 0 below 1"), ("cap", 0, "cap 0 outside 1 .. 8192"), ("cap", 8193, "cap 8193 outside 1 .. 8192"),
                                    ("lcap", 0, "lcap 0 outside 1 .. 256"), ("lcap", 257, "lcap 257 outside 1 .. 256"),
                                    ("pcap", 0, "pcap 0 outside 1 .. 64"), ("pcap", 65, "pcap 65 outside 1 .. 64"),
                                    ("n_tab", 0, "n_tab 0 outside 1 .. 4096"), ("n_tab", 4097, "n_tab 4097 outside 1 .. 4096"),
                                    ("n_pts", 0, "n_pts 0 outside 1 .. 1048576"), ("n_pts", (1 << 20) + 1, "n_pts 1048577 outside 1 .. 1048576"),
                                    ("n_lines", 0, "n_lines 0 outside 1 .. 1048576"), ("n_lines", (1 << 20) + 1, "n_lines 1048577 outside 1 .. 1048576")]}


@pytest.mark.parametrize("entry", sorted(NAMES))
def test_every_limit_is_refused_with_the_field_named(scene, entry):
    from manhattanslam_amd import _header
    assert {l[0] for l in LIMITS[entry]} == {n for t, n in _header.declarations(_header.text("msl.h"))[entry][1][1:] if t == "int"}
    for field, value, msg in LIMITS[entry]:
        assert refused(entry, scene, **{field: value}) == f"{entry}: {msg}"
    if entry == "msl_points_3d":
        assert refused(entry, scene, params=put("nlevels", 17)) == f"{entry}: nlevels 17 outside 1 .. 16"
        assert refused(entry, scene, params=put("nlevels", 0)) == f"{entry}: nlevels 0 outside 1 .. 16"
        assert refused(entry, scene, params=put("min_points", -1)) == f"{entry}: min_points -1 below 0"


@pytest.mark.parametrize("entry", sorted(NAMES))
def test_every_null_is_refused_with_the_field_named(scene, entry):
    from manhattanslam_amd import _header
    pointers = [n for t, n in _header.declarations(_header.text("msl.h"))[entry][1][1:] if t.endswith("*") and n not in ("enable", "first_id")]
    assert len(pointers) == {"msl_points_3d": 18, "msl_keyframe_decision": 29}[entry]
    for n in pointers:
        assert refused(entry, scene, **{n: None}) == f"{entry}: {n} is NULL"


def test_index_defects_of_a_host_memory_call_are_refused(scene):
    p3, kd = "msl_points_3d", "msl_keyframe_decision"
    assert refused(p3, scene, n_kps=put(1, 7)) == f"{p3}: n_kps[1] is 7 outside 0 .. 6"
    assert refused(p3, scene, n_kps=put(0, -1)) == f"{p3}: n_kps[0] is -1 outside 0 .. 6"
    assert refused(p3, scene, n_kps=put(0, -1), mode=km.ALL) == f"{p3}: n_kps[0] is -1 outside 0 .. 6"
    assert refused(p3, scene, cur_held=put((0, 2), ks.N_PTS)) == f"{p3}: cur_held[0][2] is {ks.N_PTS} of {ks.N_PTS}"
    assert refused(p3, scene, cur_held=put((1, 0), -2)) == f"{p3}: cur_held[1][0] is -2 of {ks.N_PTS}"
    assert refused(kd, scene, n_cur=put(0, 7)) == f"{kd}: n_cur[0] is 7 outside 0 .. 6"
    assert refused(kd, scene, cur_held=put((0, 0), ks.N_PTS)) == f"{kd}: cur_held[0][0] is {ks.N_PTS} of {ks.N_PTS}"
    assert refused(kd, scene, n_cur_lines=put(1, 5)) == f"{kd}: n_cur_lines[1] is 5 outside 0 .. 4"
    assert refused(kd, scene, cur_lheld=put((1, 3), ks.N_LINES)) == f"{kd}: cur_lheld[1][3] is {ks.N_LINES} of {ks.N_LINES}"
    assert refused(kd, scene, n_kps=put(2, 9)) == f"{kd}: n_kps[2] is 9 outside 0 .. 6"
    assert refused(kd, scene, held_id=put((2, 1), -4)) == f"{kd}: held_id[2][1] is -4 of {ks.N_PTS}"
    assert refused(kd, scene, n_planes=put(1, 3)) == f"{kd}: n_planes[1] is 3 outside 0 .. 2"
    assert refused(kd, scene, frames=put(1, tuple([1, 100, 95, 0, 10, 5, 0, 1, 0, 0]))) == f"{kd}: frames[1].ref_kf is keyframe 5 of 5"
    assert refused(kd, scene, frames=put(0, tuple([1, 100, 95, 0, 10, -2, 0, 1, 0, 0]))) == f"{kd}: frames[0].ref_kf is keyframe -2 of 5"


def test_the_handle_forms_refuse_a_null_handle():
    from manhattanslam_amd import _lib
    for entry, count in NAMES.items():
        args = [0 if t in (C.c_int, C.c_uint) else None for t in _lib.SIGNATURES[entry][1][1:]]
        assert len(args) == count - 1 and getattr(_lib.lib, entry)(None, *args) == -1
        assert _lib.lib.msl_last_error().decode() == f"{entry}: h is NULL"

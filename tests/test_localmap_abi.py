"""msl_local_keyframes, msl_local_points and msl_local_lines are part of the C ABI: exported by libmsl.so, declared in include/msl.h (the
budget hook in include/msl_debug.h) and bound in _lib; the two forms differ in their first argument only.  Their refusals, through the
device-indexed forms on host memory, which check before they touch a device: every limit, every NULL and every index defect of a
host-memory call is refused with the field named, and the outputs keep their bytes.  No launch (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import abi_refusals
from tests import localmap_scenes as ls
from tests.abi_refusals import put

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"msl_local_keyframes": 26, "msl_local_points": 28, "msl_local_lines": 29}


def test_exported_declared_and_bound():
    from manhattanslam_amd import _header, _lib
    dll = C.CDLL(_lib.LIB_PATH)
    src = _header.text("msl.h")
    decl, dbg = _header.declarations(src), _header.declarations(_header.text("msl_debug.h"))
    for base, count in NAMES.items():
        for n in (base, base + "_batch"):
            assert decl[n][0] == "int" and hasattr(dll, n), n
            res, args = _lib.SIGNATURES[n]
            assert res is C.c_int and len(args) == len(decl[n][1]) == count, n
            assert getattr(_lib.lib, n).argtypes == args
        a, b = decl[base][1], decl[base + "_batch"][1]
        assert a[0] == ("msl_match *", "h") and b[0] == ("int", "device") and a[1:] == b[1:]
    n = "msl_debug_local_map_budget"
    assert hasattr(dll, n) and [t for t, _ in dbg[n][1]] == ["msl_match *", "size_t"] and n not in decl
    assert not re.findall(r"msl_\w*debug\w*", src)                         # the drop-in header carries no debug name
    assert re.search(r"#define\s+MSL_LOCALMAP_NO_VOTES\s+1\b", src)


def test_argument_order_is_the_wrapper_s():
    import manhattanslam_amd as m
    from manhattanslam_amd import _header, localmap
    from tests import localmap_model as lm
    assert m.localmap is localmap and localmap.NO_VOTES == lm.NO_VOTES == 1
    assert (localmap.LOCAL_KF_STOP, localmap.BEST_COVIS) == (lm.LOCAL_KF_STOP, lm.BEST_COVIS) == (80, 10)
    decl = _header.declarations(_header.text("msl.h"))
    names = [x[1] for x in decl["msl_local_keyframes"][1]]
    assert names[1:7] == ["n_frames", "cap", "n_tab", "n_pts", "n_obs_total", "ccap"] and tuple(names[7:18]) == localmap.KF_IN_KEYS
    assert names[18] == "mem" and tuple(names[19:25]) == localmap.KF_OUT_KEYS and names[25] == "out_mem"
    names = [x[1] for x in decl["msl_local_points"][1]]
    assert names[1:6] == ["n_frames", "n_tab", "cap", "n_pts", "mcap"] and tuple(names[6:18]) == localmap.POINT_IN_KEYS
    assert names[18] == "mem" and tuple(names[19:27]) == localmap.POINT_OUT_KEYS and names[27] == "out_mem"
    names = [x[1] for x in decl["msl_local_lines"][1]]
    assert names[1:7] == ["n_frames", "n_tab", "klcap", "lcap", "n_lines", "mlcap"] and tuple(names[7:19]) == localmap.LINE_IN_KEYS
    assert names[19] == "mem" and tuple(names[20:28]) == localmap.LINE_OUT_KEYS and names[28] == "out_mem"
    # the outputs of the two gathers are, name for name, what the matchers read
    for entry, matcher in (("msl_local_points", "msl_match_local_points"), ("msl_local_lines", "msl_match_local_lines")):
        out = {n: t for t, n in decl[entry][1][-9:-1]}
        read = {n: t for t, n in decl[matcher][1]}
        assert [k for k in out if k not in read] == [decl[entry][1][-9][1]]     # local_id / local_line_id alone is new
        assert all(read[k] == "const " + t for k, t in out.items() if k in read)


def test_limits_are_the_header_s():
    from manhattanslam_amd import localmap
    text = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", "msl.h")).read())
    line = re.search(r"Local-map limits: n_frames >= 1, n_tab <= (\d+), cap <= (\d+), klcap <= (\d+), lcap <= (\d+), n_pts <= (\d+), n_lines <= (\d+), "
                     r"mcap <= (\d+), mlcap <= (\d+), 1 <= ccap <= n_tab", text)
    assert tuple(int(x) for x in line.groups()) == (localmap.MAX_TAB, localmap.MAX_CAP, localmap.MAX_KLCAP, localmap.MAX_KLCAP, localmap.MAX_PTS,
                                                    localmap.MAX_LINES, localmap.MAX_MCAP, localmap.MAX_MCAP)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    s = ls.random_scene(4, 6, 5, n_pts=20, frame_sizes=[5, 3], klcap=3, lcap=3, n_lines=5)
    s["conn"][0], s["parent"][3] = [1, 2, 3], 1
    s["frames"][0]["prev"], s["frames"][0]["held"][0], s["frames"][0]["lheld"] = [2, 4], 7, [1, None, 0]
    a, sh = ls.pack(s, cap=5, klcap=3, lcap=3)
    w = ls.model(s)
    a["local_kf"] = ls._rows([x["kf"]["local_kf"] for x in w], 6)
    a["n_local_kf"] = np.array([len(x["kf"]["local_kf"]) for x in w], np.int32)
    a["local_kf"][0], a["n_local_kf"][0] = [1, 3, -1, -1, -1, -1], 2
    return a, dict(sh, mcap=8, mlcap=4)


def refused(entry, scene, **over):
    from manhattanslam_amd import localmap
    a, sh = scene
    F = sh["n_frames"]
    out = dict(localmap.keyframes_outputs(F, sh["cap"], sh["n_tab"], ls.host_filled), **localmap.points_outputs(F, sh["cap"], sh["mcap"], ls.host_filled),
               **localmap.lines_outputs(F, sh["lcap"], sh["mlcap"], ls.host_filled))
    return abi_refusals.refused(entry, sh, a, out, **over)


LIMITS = [("n_frames", 0, "n_frames 0 below 1"), ("n_frames", -3, "n_frames -3 below 1"), ("n_tab", 0, "n_tab 0 outside 1 .. 4096"),
          ("n_tab", 4097, "n_tab 4097 outside 1 .. 4096"), ("cap", 0, "cap 0 outside 1 .. 8192"), ("cap", 8193, "cap 8193 outside 1 .. 8192"),
          ("n_pts", 0, "n_pts 0 outside 1 .. 1048576"), ("n_pts", (1 << 20) + 1, "n_pts 1048577 outside 1 .. 1048576"),
          ("n_obs_total", -1, "n_obs_total -1 below 0"), ("ccap", 0, "ccap 0 outside 1 .. n_tab = 6"), ("ccap", 7, "ccap 7 outside 1 .. n_tab = 6"),
          ("mcap", 0, "mcap 0 outside 1 .. 32768"), ("mcap", 32769, "mcap 32769 outside 1 .. 32768"), ("klcap", 0, "klcap 0 outside 1 .. 256"),
          ("klcap", 257, "klcap 257 outside 1 .. 256"), ("lcap", 0, "lcap 0 outside 1 .. 256"), ("lcap", 257, "lcap 257 outside 1 .. 256"),
          ("n_lines", 0, "n_lines 0 outside 1 .. 1048576"), ("n_lines", (1 << 20) + 1, "n_lines 1048577 outside 1 .. 1048576"),
          ("mlcap", 0, "mlcap 0 outside 1 .. 32768"), ("mlcap", 32769, "mlcap 32769 outside 1 .. 32768")]


@pytest.mark.parametrize("entry", sorted(NAMES))
def test_every_limit_is_refused_with_the_field_named(scene, entry):
    from manhattanslam_amd import _header
    names = [n for _, n in _header.declarations(_header.text("msl.h"))[entry][1]]
    mine = [l for l in LIMITS if l[0] in names]
    assert {l[0] for l in mine} == {n for t, n in _header.declarations(_header.text("msl.h"))[entry][1][1:] if t == "int"}
    for field, value, msg in mine:
        assert refused(entry, scene, **{field: value}) == f"{entry}: {msg}"


@pytest.mark.parametrize("entry", sorted(NAMES))
def test_every_null_is_refused_with_the_field_named(scene, entry):
    from manhattanslam_amd import _header
    for t, n in _header.declarations(_header.text("msl.h"))[entry][1][1:]:
        if not t.endswith("*") or n in ("prev_kf", "n_prev"):
            continue
        assert refused(entry, scene, **{n: None}) == f"{entry}: {n} is NULL"
    if entry == "msl_local_keyframes":
        assert refused(entry, scene, n_prev=None) == f"{entry}: n_prev is NULL with prev_kf given"


def test_index_defects_of_a_host_memory_call_are_refused(scene):
    kf, pts, lns = sorted(NAMES)[0], "msl_local_points", "msl_local_lines"
    assert kf == "msl_local_keyframes"
    for entry in (kf, pts):
        assert refused(entry, scene, cur_held=put((0, 0), 20)) == f"{entry}: cur_held[0][0] is 20 of 20"
        assert refused(entry, scene, cur_held=put((1, 2), -2)) == f"{entry}: cur_held[1][2] is -2 of 20"
        assert refused(entry, scene, n_cur=put(1, 6)) == f"{entry}: n_cur[1] is 6 outside 0 .. 5"
    assert refused(kf, scene, n_cur=put(0, -1)) == f"{kf}: n_cur[0] is -1 outside 0 .. 5"
    assert refused(kf, scene, parent=put(3, 6)) == f"{kf}: parent[3] is keyframe 6 of 6"
    assert refused(kf, scene, parent=put(3, -2)) == f"{kf}: parent[3] is keyframe -2 of 6"
    assert refused(kf, scene, parent=put(3, 3)) == f"{kf}: parent[3] is the keyframe itself"
    assert refused(kf, scene, conn=put((0, 1), 6)) == f"{kf}: conn[0][1] is keyframe 6 of 6"
    assert refused(kf, scene, conn=put((0, 2), -1)) == f"{kf}: conn[0][2] is keyframe -1 of 6"
    ccap = scene[1]["ccap"]
    assert refused(kf, scene, n_conn=put(2, ccap + 1)) == f"{kf}: n_conn[2] is {ccap + 1} outside 0 .. ccap = {ccap}"
    assert refused(kf, scene, prev_kf=put((0, 1), 2)) == f"{kf}: prev_kf[0] holds keyframe 2 twice"
    assert refused(kf, scene, prev_kf=put((0, 0), 6)) == f"{kf}: prev_kf[0][0] is keyframe 6 of 6"
    assert refused(kf, scene, n_prev=put(1, 7)) == f"{kf}: n_prev[1] is 7 outside 0 .. n_tab = 6"
    assert refused(kf, scene, obs_kf=put(0, 6)) == f"{kf}: obs_kf[0] is keyframe 6 of 6"
    assert refused(kf, scene, obs_off=put(3, 1000)).startswith(f"{kf}: obs_off descends at point 3")
    for entry in (pts, lns):
        assert refused(entry, scene, local_kf=put((0, 1), 1)) == f"{entry}: local_kf[0] holds keyframe 1 twice"
        assert refused(entry, scene, local_kf=put((0, 0), 6)) == f"{entry}: local_kf[0][0] is keyframe 6 of 6"
        assert refused(entry, scene, local_kf=put((0, 1), -1)) == f"{entry}: local_kf[0][1] is keyframe -1 of 6"
        assert refused(entry, scene, n_local_kf=put(1, 7)) == f"{entry}: n_local_kf[1] is 7 outside 0 .. n_tab = 6"
    assert refused(lns, scene, cur_lheld=put((0, 0), 5)) == f"{lns}: cur_lheld[0][0] is 5 of 5"
    assert refused(lns, scene, n_cur_lines=put(0, 4)) == f"{lns}: n_cur_lines[0] is 4 outside 0 .. 3"


def test_the_handle_forms_refuse_a_null_handle():
    from manhattanslam_amd import _lib
    for entry, count in NAMES.items():
        args = [0 if t in (C.c_int, C.c_uint) else None for t in _lib.SIGNATURES[entry][1][1:]]
        assert len(args) == count - 1 and getattr(_lib.lib, entry)(None, *args) == -1
        assert _lib.lib.msl_last_error().decode() == f"{entry}: h is NULL"
    assert _lib.lib.msl_debug_local_map_budget(None, 1 << 20) == -1

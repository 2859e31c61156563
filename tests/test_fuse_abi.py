"""msl_fuse_candidates and msl_fuse_map_points are part of the C ABI: exported by libmsl.so, declared in include/msl.h (the debug accessor in
include/msl_debug.h) and bound in _lib with matching argument types; the two forms differ in their first argument only; the params record
and the status codes have the header's layout and values.  No compute calls (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"msl_fuse_candidates": 16, "msl_fuse_candidates_batch": 16, "msl_fuse_map_points": 32, "msl_fuse_map_points_batch": 32}
CODES = ("NULL", "BAD", "IN_KEYFRAME", "BEHIND", "OUT_OF_IMAGE", "DISTANCE", "VIEW_ANGLE", "NO_FEATURE", "NO_CANDIDATE", "ABOVE_TH_LOW", "ADDED",
         "REPLACED_BY_HELD", "REPLACES_HELD", "HELD_BAD", "UNRESOLVED")


def test_exported_declared_and_bound():
    from manhattanslam_amd import _header, _lib
    dll = C.CDLL(_lib.LIB_PATH)
    src = _header.text("msl.h")
    decl, dbg = _header.declarations(src), _header.declarations(_header.text("msl_debug.h"))
    for n, count in NAMES.items():
        assert decl[n][0] == "int", n
        assert hasattr(dll, n), n
        res, args = _lib.SIGNATURES[n]
        assert res is C.c_int and len(args) == len(decl[n][1]) == count, n        # the types: test_abi.py, against the compiler
        assert getattr(_lib.lib, n).argtypes == args
    n = "msl_debug_fuse"
    assert hasattr(dll, n) and len(_lib.SIGNATURES[n][1]) == len(dbg[n][1]) == 4
    assert "fuse" not in " ".join(re.findall(r"msl_\w*debug\w*", src))                 # the accessor is not part of the drop-in header


def test_argument_order_of_the_two_forms():
    from manhattanslam_amd import _header, fuse
    decl = _header.declarations(_header.text("msl.h"))
    a, b = decl["msl_fuse_map_points"][1], decl["msl_fuse_map_points_batch"][1]
    assert a[0] == ("msl_match *", "h") and b[0] == ("int", "device") and a[1:] == b[1:]
    names = [x[1] for x in a]
    assert names[1:8] == ["n_tab", "cap", "n_pts", "n_items", "n_lists", "lcap", "params"]
    assert tuple(names[8:15]) == fuse.TABLE_KEYS and tuple(names[15:21]) == fuse.POINT_KEYS
    assert names[21:26] == ["tgt", "list", "cand", "n_cand", "mem"] and tuple(names[26:31]) == fuse.OUT_KEYS and names[31] == "out_mem"
    assert a[8][0] == "const msl_keypoint *" and a[28][0] == "uint8_t *" and a[26][0] == "int32_t *"
    a, b = decl["msl_fuse_candidates"][1], decl["msl_fuse_candidates_batch"][1]
    assert a[0] == ("msl_match *", "h") and b[0] == ("int", "device") and a[1:] == b[1:]
    names = [x[1] for x in a]
    assert names[1:] == ["n_tab", "cap", "n_pts", "n_items", "tcap", "lcap", "held_id", "n_kps", "pt_flags", "targets", "n_targets", "mem", "cand",
                         "n_cand", "out_mem"]


def test_params_record_and_status_codes():
    from manhattanslam_amd import _header, _lib, fuse
    d = _lib.FUSE_PARAMS_DTYPE
    src = _header.text("msl.h")
    assert _header.records(src)["msl_fuse_params"].names == d.names
    off = {n: d.fields[n][1] for n in d.names}
    assert off == dict(fx=0, fy=4, cx=8, cy=12, bf=16, minX=20, maxX=24, minY=28, maxY=32, th=36, nlevels=40, scale_factors=44, inv_level_sigma2=108,
                       log_scale_factor=172, th_low=176) and d.itemsize == 180
    assert re.search(r"#define\s+MSL_MATCH_MAX_LEVELS\s+16\b", src) and d.fields["scale_factors"][0].shape == (16,)
    from tests import fuse_model as fm
    assert fm.CODES == CODES
    for v, k in enumerate(CODES):
        assert re.search(r"#define\s+MSL_FUSE_" + k + r"\s+" + str(v) + r"\b", src), k
        assert getattr(fuse, k) == v and getattr(fm, k) == v
    assert len(re.findall(r"#define\s+MSL_FUSE_\w+", src)) == len(CODES)


def test_limits_are_the_header_s():
    from manhattanslam_amd import fuse
    text = open(os.path.join(ROOT, "include", "msl.h")).read()
    line = re.search(r"Limits: cap <= (\d+), n_tab <= (\d+), n_pts <= (\d+), lcap <= (\d+), tcap <= (\d+), n_items <= (\d+)", text)
    assert tuple(int(x) for x in line.groups()) == (fuse.MAX_CAP, fuse.MAX_TAB, fuse.MAX_PTS, fuse.MAX_LCAP, fuse.MAX_TCAP, fuse.MAX_ITEMS)


def test_python_wrapper_is_exported():
    import manhattanslam_amd as m
    from manhattanslam_amd import fuse
    assert m.fuse is fuse and m.FUSE_PARAMS_DTYPE is m._lib.FUSE_PARAMS_DTYPE
    assert all(callable(getattr(fuse, n)) for n in ("fuse_params", "fuse_candidates", "fuse_candidates_device", "fuse_map_points",
                                                    "fuse_map_points_device", "debug_fuse", "pack_table", "pack_points", "pack_lists"))
    from tests import fuse_scenes as fs
    want = fs.prm()
    p = fuse.fuse_params(fs.FX, fs.FY, fs.CX, fs.CY, fs.BF, 0.0, fs.W, 0.0, fs.H, want["scale_factors"], want["inv_level_sigma2"], want["log_scale_factor"])
    for k in ("fx", "fy", "cx", "cy", "bf", "minX", "maxX", "minY", "maxY", "th", "log_scale_factor"):
        assert p[k][0] == want[k], k
    assert p["nlevels"][0] == 8 and p["th_low"][0] == 50 and p["th"][0] == 3.0
    assert (p["scale_factors"][0, :8] == want["scale_factors"]).all() and (p["inv_level_sigma2"][0, :8] == want["inv_level_sigma2"]).all()
    assert not p["scale_factors"][0, 8:].any()
    assert np.dtype(m.FUSE_PARAMS_DTYPE).itemsize == 180

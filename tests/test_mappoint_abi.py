"""msl_refresh_map_points and msl_covisibility are part of the C ABI: exported by libmsl.so, declared in include/msl.h and bound in _lib with
matching argument types; the two forms differ in their first argument only; the params record, the mask and the status bits have the
header's layout and values.  No compute calls (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"msl_refresh_map_points": 31, "msl_refresh_map_points_batch": 31, "msl_covisibility": 20, "msl_covisibility_batch": 20}


def test_exported_declared_and_bound():
    from manhattanslam_amd import _header, _lib
    dll = C.CDLL(_lib.LIB_PATH)
    src = _header.text("msl.h")
    decl = _header.declarations(src)
    for n, count in NAMES.items():
        assert decl[n][0] == "int", n
        assert hasattr(dll, n), n
        res, args = _lib.SIGNATURES[n]
        assert res is C.c_int and len(args) == len(decl[n][1]) == count, n        # the types: test_abi.py, against the compiler
        assert getattr(_lib.lib, n).argtypes == args


def test_argument_order_of_the_two_forms():
    from manhattanslam_amd import _header, mappoint
    decl = _header.declarations(_header.text("msl.h"))
    a, b = decl["msl_refresh_map_points"][1], decl["msl_refresh_map_points_batch"][1]
    assert a[0] == ("msl_match *", "h") and b[0] == ("int", "device") and a[1:] == b[1:]
    names = [x[1] for x in a]
    assert names[1:8] == ["n_tab", "cap", "n_pts", "n_items", "n_obs_total", "what", "params"]
    assert tuple(names[8:13]) == mappoint.TABLE_KEYS and tuple(names[13:16]) == mappoint.OBS_KEYS and tuple(names[16:19]) == mappoint.POINT_KEYS
    assert names[19:21] == ["ids", "mem"] and tuple(names[21:27]) == mappoint.OUT_KEYS and tuple(names[27:30]) == mappoint.ROW_KEYS
    assert names[30] == "out_mem"
    assert a[8][0] == "const msl_keypoint *" and a[21][0] == "uint8_t *" and a[26][0] == "uint8_t *" and a[22][0] == "float *"
    a, b = decl["msl_covisibility"][1], decl["msl_covisibility_batch"][1]
    assert a[0] == ("msl_match *", "h") and b[0] == ("int", "device") and a[1:] == b[1:]
    names = [x[1] for x in a]
    assert names[1:15] == ["n_tab", "cap", "n_pts", "n_items", "n_obs_total", "ccap", "th", "held_id", "n_kps", "pt_flags", "obs_off", "obs_kf", "kf",
                           "mem"]
    assert tuple(names[15:19]) == mappoint.COVIS_KEYS and names[19] == "out_mem"


def test_params_record_mask_and_status_bits():
    from manhattanslam_amd import _header, _lib, mappoint
    from tests import mappoint_model as mm
    d = _lib.REFRESH_PARAMS_DTYPE
    src = _header.text("msl.h")
    assert _header.records(src)["msl_refresh_params"].names == d.names == ("nlevels", "scale_factors")
    assert d.fields["nlevels"][1] == 0 and d.fields["scale_factors"][1] == 4 and d.itemsize == 68
    assert re.search(r"#define\s+MSL_MATCH_MAX_LEVELS\s+16\b", src) and d.fields["scale_factors"][0].shape == (16,)
    want = dict(DESC=1, NORMAL=2, DESC_WRITTEN=1, NORMAL_WRITTEN=2, BAD=4, NO_OBS=8, NO_LIVE_KF=16, TOO_MANY=32, BAD_OCTAVE=64)
    for k, v in want.items():
        assert re.search(r"#define\s+MSL_REFRESH_" + k + r"\s+" + str(v) + r"\b", src), k
        py = "REFRESH_" + k if k in ("DESC", "NORMAL") else k
        assert getattr(mappoint, py) == v and getattr(mm, py) == v
    assert len(re.findall(r"#define\s+MSL_REFRESH_\w+", src)) == len(want)
    assert mm.BITS == tuple(k for k in want if k not in ("DESC", "NORMAL"))
    assert re.search(r"#define\s+MSL_OBS_MAX\s+256\b", src) and mappoint.OBS_MAX == mm.OBS_MAX == 256


def test_limits_are_the_header_s():
    from manhattanslam_amd import mappoint
    text = open(os.path.join(ROOT, "include", "msl.h")).read()
    line = re.search(r"Limits: n_tab <= (\d+), cap <= (\d+), n_pts <= (\d+), n_items <= n_pts \(refresh\) / <= n_tab \(covisibility\), ccap <= n_tab", text)
    assert tuple(int(x) for x in line.groups()) == (mappoint.MAX_TAB, mappoint.MAX_CAP, mappoint.MAX_PTS)


def test_python_wrapper_is_exported():
    import manhattanslam_amd as m
    from manhattanslam_amd import mappoint
    from tests import mappoint_model as mm
    assert m.mappoint is mappoint and m.REFRESH_PARAMS_DTYPE is m._lib.REFRESH_PARAMS_DTYPE
    assert all(callable(getattr(mappoint, n)) for n in mappoint.__all__ if n[0].islower())
    want = mm.params()
    p = mappoint.refresh_params(want["scale_factors"])
    assert p["nlevels"][0] == 8 and (p["scale_factors"][0, :8] == want["scale_factors"]).all() and not p["scale_factors"][0, 8:].any()
    assert np.dtype(m.REFRESH_PARAMS_DTYPE).itemsize == 68

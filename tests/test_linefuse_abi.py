"""msl_fuse_map_lines and msl_refresh_map_lines are part of the C ABI: exported by libmsl.so, declared in include/msl.h (the debug accessor
in include/msl_debug.h) and bound in _lib with matching argument types; the two forms differ in their first argument only; the params
record and the status codes have the header's layout and values.  No compute calls (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"msl_fuse_map_lines": 30, "msl_fuse_map_lines_batch": 30, "msl_refresh_map_lines": 24, "msl_refresh_map_lines_batch": 24}
CODES = ("NULL", "BAD", "BEHIND", "OUT_OF_IMAGE", "DISTANCE", "VIEW_ANGLE", "NO_FEATURE", "NO_CANDIDATE", "ABOVE_TH_LOW", "ADDED", "REPLACED_BY_HELD",
         "REPLACES_HELD", "HELD_BAD", "UNRESOLVED", "SELF")


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
    n = "msl_debug_line_fuse"
    assert hasattr(dll, n) and len(_lib.SIGNATURES[n][1]) == len(dbg[n][1]) == 4
    assert not re.findall(r"msl_\w*debug\w*", src)                                   # the accessor is not part of the drop-in header


def test_argument_order_of_the_two_forms():
    from manhattanslam_amd import _header, linefuse
    decl = _header.declarations(_header.text("msl.h"))
    a, b = decl["msl_fuse_map_lines"][1], decl["msl_fuse_map_lines_batch"][1]
    assert a[0] == ("msl_match *", "h") and b[0] == ("int", "device") and a[1:] == b[1:]
    names = [x[1] for x in a]
    assert names[1:8] == ["n_tab", "klcap", "n_lines", "n_items", "n_lists", "lcap", "params"]
    assert tuple(names[8:13]) == linefuse.TABLE_KEYS and tuple(names[13:19]) == linefuse.LINE_KEYS
    assert names[19:24] == ["tgt", "list", "cand", "n_cand", "mem"] and tuple(names[24:29]) == linefuse.OUT_KEYS and names[29] == "out_mem"
    assert a[8][0] == "const msl_keyline *" and a[13][0] == "const double *" and a[26][0] == "uint8_t *"
    a, b = decl["msl_refresh_map_lines"][1], decl["msl_refresh_map_lines_batch"][1]
    assert a[0] == ("msl_match *", "h") and b[0] == ("int", "device") and a[1:] == b[1:]
    names = [x[1] for x in a]
    assert names[1:7] == ["n_tab", "klcap", "n_lines", "n_items", "n_obs_total", "params"]
    assert tuple(names[7:10]) == linefuse.REFRESH_TABLE_KEYS and tuple(names[10:13]) == linefuse.OBS_KEYS
    assert tuple(names[13:16]) == linefuse.REFRESH_LINE_KEYS and names[16:18] == ["ids", "mem"]
    assert tuple(names[18:21]) == linefuse.REFRESH_OUT_KEYS and tuple(names[21:23]) == linefuse.ROW_KEYS and names[23] == "out_mem"
    assert a[18][0] == "double *" and a[21][0] == "double *" and a[6][0] == "const msl_refresh_params *"


def test_params_record_and_status_codes():
    from manhattanslam_amd import _header, _lib, linefuse
    d = _lib.LINE_FUSE_PARAMS_DTYPE
    src = _header.text("msl.h")
    assert _header.records(src)["msl_line_fuse_params"].names == d.names
    off = {n: d.fields[n][1] for n in d.names}
    assert off == dict(fx=0, fy=4, cx=8, cy=12, minX=16, maxX=20, minY=24, maxY=28, th=32, nlevels=36, scale_factors=40, log_scale_factor=104,
                       th_low=108) and d.itemsize == 112
    assert d.fields["scale_factors"][0].shape == (16,)
    from tests import linefuse_model as lf
    assert lf.CODES == CODES
    for v, k in enumerate(CODES):
        assert re.search(r"#define\s+MSL_LFUSE_" + k + r"\s+" + str(v) + r"\b", src), k
        assert getattr(linefuse, k) == v and getattr(lf, k) == v
    assert len(re.findall(r"#define\s+MSL_LFUSE_\w+", src)) == len(CODES)
    assert linefuse.INT_MAX == lf.INT_MAX == 2 ** 31 - 1
    for k, bit in (("NORMAL_WRITTEN", lf.NORMAL_WRITTEN), ("BAD", lf.R_BAD), ("NO_OBS", lf.NO_OBS), ("BAD_OCTAVE", lf.BAD_OCTAVE)):
        assert re.search(r"#define\s+MSL_REFRESH_" + k + r"\s+" + str(bit) + r"\b", src), k


def test_limits_are_the_header_s():
    from manhattanslam_amd import linefuse
    text = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", "msl.h")).read())
    line = re.search(r"Limits: klcap <= (\d+), n_tab <= (\d+), n_lines <= (\d+), lcap <= (\d+), n_items <= (\d+), nlevels <= MSL_MATCH_MAX_LEVELS, "
                     r"0 <= th_low <= (\d+)", text)
    assert tuple(int(x) for x in line.groups()) == (linefuse.MAX_KLCAP, linefuse.MAX_TAB, linefuse.MAX_LINES, linefuse.MAX_LCAP, linefuse.MAX_ITEMS, 256)
    line = re.search(r"Refresh limits: n_tab <= (\d+), klcap <= (\d+), n_lines <= (\d+), n_items <= n_lines", text)
    assert tuple(int(x) for x in line.groups()) == (linefuse.MAX_TAB, linefuse.MAX_KLCAP, linefuse.MAX_LINES)


def test_python_wrapper_is_exported():
    import manhattanslam_amd as m
    from manhattanslam_amd import linefuse
    assert m.linefuse is linefuse and m.LINE_FUSE_PARAMS_DTYPE is m._lib.LINE_FUSE_PARAMS_DTYPE
    assert all(callable(getattr(linefuse, n)) for n in ("line_fuse_params", "pack_line_table", "pack_lines", "fuse_map_lines", "fuse_map_lines_device",
                                                        "refresh_map_lines", "refresh_map_lines_device", "debug_line_fuse"))
    from tests import linefuse_scenes as ls
    want = ls.prm()
    p = linefuse.line_fuse_params(ls.FX, ls.FY, ls.CX, ls.CY, 0.0, ls.W, 0.0, ls.H, want["scale_factors"], want["log_scale_factor"])
    for k in ("fx", "fy", "cx", "cy", "minX", "maxX", "minY", "maxY", "th", "log_scale_factor"):
        assert p[k][0] == want[k], k
    assert p["nlevels"][0] == 8 and p["th_low"][0] == 50 and p["th"][0] == 3.0
    assert (p["scale_factors"][0, :8] == want["scale_factors"]).all() and not p["scale_factors"][0, 8:].any()
    assert np.dtype(m.LINE_FUSE_PARAMS_DTYPE).itemsize == 112

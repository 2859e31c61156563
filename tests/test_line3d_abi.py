"""msl_lines_3d is part of the C ABI: exported by libmsl.so, declared in include/msl.h (its debug accessor in include/msl_debug.h) and bound in
_lib with matching argument types, and the params record has the header's layout.  No compute calls (no GPU needed)."""
import ctypes as C
import re

import numpy as np

NAMES = ("msl_lines_3d", "msl_lines_3d_batch")


def test_exported_declared_and_bound():
    from manhattanslam_amd import _header, _lib
    dll = C.CDLL(_lib.LIB_PATH)
    src = _header.text("msl.h")
    decl, dbg = _header.declarations(src), _header.declarations(_header.text("msl_debug.h"))
    for n in NAMES:
        assert decl[n][0] == "int", n
        assert hasattr(dll, n), n
        res, args = _lib.SIGNATURES[n]
        assert res is C.c_int and len(args) == len(decl[n][1]) == 23, n                 # the types: test_abi.py, against the compiler
        assert args.count(C.c_size_t) == 2 and args[8] is C.c_size_t and args[9] is C.c_size_t      # the depth strides
        assert getattr(_lib.lib, n).argtypes == args
    n = "msl_lines_3d_debug"
    assert hasattr(dll, n) and len(_lib.SIGNATURES[n][1]) == len(dbg[n][1])
    assert decl[NAMES[0]][1][0] == ("msl_match *", "h") and decl[NAMES[1]][1][0] == ("int", "device")
    for k, v in (("MSL_LINE3D_ALL", 0), ("MSL_LINE3D_INDEX_ORDER", 1), ("MSL_LINE3D_DEPTH_ORDER", 2)):
        assert re.search(r"#define\s+" + k + r"\s+" + str(v) + r"\b", src), k


def test_params_record_layout():
    from manhattanslam_amd import LINE3D_PARAMS_DTYPE as d
    from manhattanslam_amd import _header
    assert _header.records(_header.text("msl.h"))["msl_line3d_params"].names == d.names
    off = {n: d.fields[n][1] for n in d.names}
    assert off == dict(fx=0, fy=4, cx=8, cy=12, max_samples=16, min_points=20, max_iterations=24, max_new_lines=28, dist_thresh=32, min_support=40,
                       min_length=48) and d.itemsize == 56
    assert all(d.fields[n][0] == np.dtype("<f8") for n in ("dist_thresh", "min_support", "min_length"))


def test_python_wrapper_is_exported():
    import manhattanslam_amd as m
    from manhattanslam_amd import line3d
    assert m.line3d is line3d and all(callable(getattr(line3d, n)) for n in ("line3d_params", "lines_3d", "lines_3d_device", "debug_lines"))
    assert (line3d.ALL, line3d.INDEX_ORDER, line3d.DEPTH_ORDER) == (0, 1, 2)
    p = line3d.line3d_params(525.0, 526.0, 319.5, 239.5)
    assert (p["fx"][0], p["fy"][0], p["cx"][0], p["cy"][0]) == (525.0, 526.0, 319.5, 239.5)
    assert (p["max_samples"][0], p["min_points"][0], p["max_iterations"][0], p["max_new_lines"][0]) == (100, 10, 10, 30)
    assert (p["dist_thresh"][0], p["min_support"][0], p["min_length"][0]) == (1.5, 0.4, 0.02)

"""msl_lines_3d is part of the C ABI: exported by libmsl.so, declared in include/msl.h (its debug accessor in include/msl_debug.h) and bound in
_lib with matching argument types, and the params record has the header's layout.  No compute calls (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("msl_lines_3d", "msl_lines_3d_batch")


def _header(name="msl.h"):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def _argtypes(src, n):
    """The ctypes argument types the header's declaration of n asks for."""
    args = re.search(r"\b" + n + r"\s*\((.*?)\)\s*MSL_NOEXCEPT", src, flags=re.S).group(1)
    return [C.c_void_p if "*" in a else (C.c_size_t if re.match(r"\s*size_t\b", a) else C.c_int) for a in args.split(",")]


def test_exported_declared_and_bound():
    from manhattanslam_amd import _lib
    dll = C.CDLL(_lib.LIB_PATH)
    src = _header()
    for n in NAMES:
        assert re.search(r"MSL_API\s+int\s+" + n + r"\s*\(", src), n
        assert hasattr(dll, n), n
        res, args = _lib.SIGNATURES[n]
        assert res is C.c_int and args == _argtypes(src, n) and len(args) == 23, n
        assert args.count(C.c_size_t) == 2 and args[8] is C.c_size_t and args[9] is C.c_size_t      # the depth strides
        assert getattr(_lib.lib, n).argtypes == args
    n = "msl_lines_3d_debug"
    assert hasattr(dll, n) and _lib.SIGNATURES[n][1] == _argtypes(_header("msl_debug.h"), n)
    first = lambda n: re.search(r"\b" + n + r"\s*\(\s*([^,]*),", src).group(1).strip()
    assert first(NAMES[0]) == "msl_match *h" and first(NAMES[1]) == "int device"
    for k, v in (("MSL_LINE3D_ALL", 0), ("MSL_LINE3D_INDEX_ORDER", 1), ("MSL_LINE3D_DEPTH_ORDER", 2)):
        assert re.search(r"#define\s+" + k + r"\s+" + str(v) + r"\b", src), k


def test_params_record_layout():
    from manhattanslam_amd import LINE3D_PARAMS_DTYPE as d
    body = re.search(r"typedef struct msl_line3d_params \{(.*?)\} msl_line3d_params;", _header(), flags=re.S).group(1)
    names = [n for decl in re.findall(r"[\w\s]+?([\w\s,\[\]]+);", body) for n in re.findall(r"(\w+)(?:\[\w+\])?\s*(?:,|$)", decl.strip())]
    assert tuple(names) == d.names, (names, d.names)
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

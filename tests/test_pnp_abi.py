"""msl_pnp_ransac is part of the C ABI: exported by libmsl.so, declared in include/msl.h (its debug accessor in include/msl_debug.h) and bound
in _lib with matching argument types, and the params record has the header's layout.  No compute calls (no GPU needed)."""
import ctypes as C

import numpy as np

NAMES = ("msl_pnp_ransac", "msl_pnp_ransac_batch")


def test_exported_declared_and_bound():
    from manhattanslam_amd import _header, _lib
    dll = C.CDLL(_lib.LIB_PATH)
    src = _header.text("msl.h")
    decl, dbg = _header.declarations(src), _header.declarations(_header.text("msl_debug.h"))
    for n in NAMES:
        assert decl[n][0] == "int", n
        assert hasattr(dll, n), n
        res, args = _lib.SIGNATURES[n]
        assert res is C.c_int and len(args) == len(decl[n][1]) == 18, n                 # the types: test_abi.py, against the compiler
        assert getattr(_lib.lib, n).argtypes == args
    n = "msl_pnp_debug_hypotheses"
    assert hasattr(dll, n) and len(_lib.SIGNATURES[n][1]) == len(dbg[n][1])
    assert decl[NAMES[0]][1][0] == ("msl_match *", "h") and decl[NAMES[1]][1][0] == ("int", "device")


def test_params_record_layout():
    from manhattanslam_amd import PNP_PARAMS_DTYPE as d
    from manhattanslam_amd import _header
    assert _header.records(_header.text("msl.h"))["msl_pnp_params"].names == d.names
    off = {n: d.fields[n][1] for n in d.names}
    assert off == dict(fx=0, fy=4, cx=8, cy=12, nlevels=16, level_sigma2=20, probability=88, min_inliers=96, max_iterations=100, min_set=104,
                       epsilon=108, th2=112, n_iterations=116) and d.itemsize == 120
    assert d.fields["probability"][0] == np.dtype("<f8") and d.fields["level_sigma2"][0].shape == (16,)


def test_python_wrapper_is_exported():
    import manhattanslam_amd as m
    from manhattanslam_amd import pnp
    assert m.pnp is pnp and all(callable(getattr(pnp, n)) for n in ("pnp_params", "pnp_ransac", "pnp_ransac_device", "debug_hypotheses"))
    p = pnp.pnp_params(525.0, 525.0, 319.5, 239.5, np.arange(1, 9, dtype=np.float32))
    assert p["nlevels"][0] == 8 and p["level_sigma2"][0, 7] == 8.0 and p["level_sigma2"][0, 8] == 0.0
    assert (p["probability"][0], p["min_inliers"][0], p["max_iterations"][0], p["min_set"][0], p["n_iterations"][0]) == (0.99, 10, 300, 4, 5)
    assert p["epsilon"][0] == np.float32(0.5) and p["th2"][0] == np.float32(5.991)

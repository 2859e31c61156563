"""msl_plane_associate[_batch] and msl_manhattan_detect[_batch] are part of the C ABI: exported by libmsl.so, declared in include/msl.h and
bound in _lib.  No compute calls (no GPU needed)."""
import ctypes as C

NAMES = ("msl_plane_associate", "msl_plane_associate_batch", "msl_manhattan_detect", "msl_manhattan_detect_batch")


def test_exported_declared_and_bound():
    from manhattanslam_amd import _header, _lib
    decl = _header.declarations(_header.text("msl.h"))
    dll = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert decl[n][0] == "int", n
        assert hasattr(dll, n), n
        assert n in _lib.SIGNATURES, n


def test_argument_counts_match_the_header():
    from manhattanslam_amd import _header, _lib
    decl = _header.declarations(_header.text("msl.h"))
    for n in NAMES:
        assert len(decl[n][1]) == len(_lib.SIGNATURES[n][1]), n


def test_params_record_is_five_floats():
    from manhattanslam_amd import PLANE_PARAMS_DTYPE
    assert PLANE_PARAMS_DTYPE.itemsize == 20 and PLANE_PARAMS_DTYPE.names == ("d_th", "a_th", "ver_th", "par_th", "mf_ver_th")

"""msl_pose_optimize_translation[_batch] are part of the C ABI: exported by libmsl.so, declared in include/msl.h and bound in _lib with the
argument list of msl_pose_optimize plus Rcw after Tcw.  No compute calls (no GPU needed)."""
import ctypes as C

NAMES = ("msl_pose_optimize_translation", "msl_pose_optimize_translation_batch")


def test_exported_declared_and_bound():
    from manhattanslam_amd import _header, _lib
    decl = _header.declarations(_header.text("msl.h"))
    dll = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert decl[n][0] == "int", n
        assert hasattr(dll, n), n
        assert n in _lib.SIGNATURES, n


def test_signature_is_pose_optimize_plus_rcw():
    from manhattanslam_amd import _lib
    for base, tr in (("msl_pose_optimize", NAMES[0]), ("msl_pose_optimize_batch", NAMES[1])):
        rb, ab = _lib.SIGNATURES[base]
        rt, at = _lib.SIGNATURES[tr]
        i = 6 + 15                                                            # handle / device, five ints, params, kps .. Tcw
        assert rt == rb and at == ab[:i] + [C.c_void_p] + ab[i:]

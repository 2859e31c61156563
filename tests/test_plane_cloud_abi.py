"""msl_plane_clouds[_batch] and msl_map_plane_merge[_batch] are part of the C ABI: exported by libmsl.so, declared in include/msl.h and
bound in _lib; the params record and the limits match the header.  No compute calls (no GPU needed)."""
import ctypes as C

NAMES = ("msl_plane_clouds", "msl_plane_clouds_batch", "msl_map_plane_merge", "msl_map_plane_merge_batch")


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
    for a, b in (NAMES[:2], NAMES[2:]):                                       # the two forms differ in their first parameter only
        assert _lib.SIGNATURES[a][1][1:] == _lib.SIGNATURES[b][1][1:]
        assert _lib.SIGNATURES[a][1][0] is C.c_void_p and _lib.SIGNATURES[b][1][0] is C.c_int


def test_params_record_and_limits_match_the_header():
    from manhattanslam_amd import PLANE_CLOUD_PARAMS_DTYPE, PLANE_PARAMS_DTYPE, _header, plane_cloud
    d = PLANE_CLOUD_PARAMS_DTYPE
    assert d.names == ("leaf", "dis_th", "max_iterations", "_pad", "probability") and d.itemsize == 24
    assert [d.fields[n][1] for n in d.names] == [0, 4, 8, 12, 16]
    assert PLANE_PARAMS_DTYPE.itemsize == 20                                  # the association's record is left as it was
    defs = _header.defines(_header.text("msl.h"))
    assert defs["MSL_PLANE_CLOUD_MAX_VOXELS"] == plane_cloud.MAX_VOXELS >= 4096
    assert defs["MSL_PLANE_CLOUD_MAX_VERTICES"] == plane_cloud.MAX_VERTICES == 1 << 17
    from tests import plane_cloud_model as pcm
    assert pcm.MAX_VOXELS == plane_cloud.MAX_VOXELS
    want = dict(KEPT=pcm.KEPT, GATE=pcm.GATE, FEW=pcm.FEW, NO_MODEL=pcm.NO_MODEL, VOXELS=pcm.VOXELS, GRID=pcm.GRID, NO_ROOM=pcm.NO_ROOM)
    for k, v in want.items():
        assert defs["MSL_PLANE_CLOUD_" + k] == v, k
    for k, v in dict(UNTOUCHED=pcm.UNTOUCHED, MERGED=pcm.MERGED, VOXELS=pcm.VOXELS, GRID=pcm.GRID, NO_ROOM=pcm.NO_ROOM).items():
        assert defs["MSL_PLANE_MERGE_" + k] == v, k
    p = plane_cloud.plane_cloud_params()
    assert float(p["leaf"][0]) == float(__import__("numpy").float32(0.2)) and int(p["max_iterations"][0]) == 50 and float(p["probability"][0]) == 0.99

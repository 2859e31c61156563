"""The keyframe-search entry points are part of the C ABI: exported by libmsl.so, declared in include/msl.h and bound in _lib, and the
params record has the header's layout.  No compute calls (no GPU needed)."""
import ctypes as C

import numpy as np

NAMES = ("msl_match_keyframe_points", "msl_match_keyframe_points_batch", "msl_kfdb_add", "msl_kfdb_erase", "msl_kfdb_clear", "msl_kfdb_size",
         "msl_reloc_candidates", "msl_reloc_candidates_batch")
COUNTS = dict(zip(NAMES, (22, 22, 7, 2, 1, 3, 16, 16)))


def test_exported_declared_and_bound():
    from manhattanslam_amd import _header, _lib
    decl = _header.declarations(_header.text("msl.h"))
    dll = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert decl[n][0] == "int", n
        assert hasattr(dll, n), n
        assert n in _lib.SIGNATURES, n
    assert decl["msl_kfdb_create"] == ("msl_kfdb *", [("int", "device")])
    assert decl["msl_kfdb_destroy"][0] == "void"
    for n in ("msl_kfdb_create", "msl_kfdb_destroy"):
        assert hasattr(dll, n) and n in _lib.SIGNATURES, n


def test_kfdb_without_a_device_fails():
    """No CPU fallback: without an MI355X msl_kfdb_create returns NULL with the no-device error."""
    import pytest
    from manhattanslam_amd import MslError, device_count
    from manhattanslam_amd.reloc import KeyFrameDatabase
    if device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(MslError, match="no HIP device|no CPU fallback"):
        KeyFrameDatabase()


def test_argument_counts_match_the_header():
    from manhattanslam_amd import _header, _lib
    decl = _header.declarations(_header.text("msl.h"))
    for n in NAMES:
        assert len(decl[n][1]) == len(_lib.SIGNATURES[n][1]) == COUNTS[n], n


def test_params_record_layout():
    """msl_keyframe_match_params = msl_match_params, then a float and an int32."""
    from manhattanslam_amd import KEYFRAME_MATCH_PARAMS_DTYPE, MATCH_PARAMS_DTYPE
    d = KEYFRAME_MATCH_PARAMS_DTYPE
    assert d.names[:len(MATCH_PARAMS_DTYPE.names)] == MATCH_PARAMS_DTYPE.names and d.names[-2:] == ("log_scale_factor", "orb_dist")
    assert d.fields["log_scale_factor"][1] == MATCH_PARAMS_DTYPE.itemsize == 112 and d.fields["orb_dist"][1] == 116 and d.itemsize == 120
    assert d.fields["orb_dist"][0] == np.dtype("<i4")
    members = [p.split(".")[0] for p in d.metadata["paths"]]                 # the C members, `base` once per flattened field
    assert members == ["base"] * len(MATCH_PARAMS_DTYPE.names) + ["log_scale_factor", "orb_dist"]


def test_python_wrapper_is_exported():
    import manhattanslam_amd as m
    from manhattanslam_amd import reloc
    assert m.reloc is reloc and callable(reloc.search_keyframe_points) and callable(reloc.keyframe_match_params)
    assert callable(reloc.reloc_candidates) and all(hasattr(reloc.KeyFrameDatabase, n) for n in ("add", "erase", "clear", "size", "close"))
    p = reloc.keyframe_match_params(np.zeros(1, _frame_params_dtype()), np.ones(8, np.float32), 10.0, 100, np.float32(0.1823))
    assert p["th"][0] == 10.0 and p["orb_dist"][0] == 100 and p["nlevels"][0] == 8 and p["check_orientation"][0] == 1


def _frame_params_dtype():
    from manhattanslam_amd._lib import FRAME_PARAMS_DTYPE
    return FRAME_PARAMS_DTYPE

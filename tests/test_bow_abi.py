"""The bag-of-words entry points are part of the C ABI: exported by libmsl.so, declared in include/msl.h and bound in _lib; the vocabulary
constructor fails loudly without a device.  No compute calls (no GPU needed)."""
import ctypes as C

import numpy as np
import pytest

NAMES = ("msl_bow_transform", "msl_bow_transform_batch", "msl_match_by_bow", "msl_match_by_bow_batch", "msl_match_lines_by_descriptor",
         "msl_match_lines_by_descriptor_batch", "msl_vocab_info")
CTORS = ("msl_vocab_create", "msl_vocab_load_text")


def test_exported_declared_and_bound():
    from manhattanslam_amd import _header, _lib
    decl = _header.declarations(_header.text("msl.h"))
    dll = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert decl[n][0] == "int", n
    for n in CTORS:
        assert decl[n][0] == "msl_vocab *", n
    assert decl["msl_vocab_destroy"][0] == "void"
    for n in NAMES + CTORS + ("msl_vocab_destroy",):
        assert hasattr(dll, n), n
        assert n in _lib.SIGNATURES, n


def test_argument_counts_match_the_header():
    from manhattanslam_amd import _header, _lib
    decl = _header.declarations(_header.text("msl.h"))
    for n in NAMES + CTORS + ("msl_vocab_destroy",):
        assert len(decl[n][1]) == len(_lib.SIGNATURES[n][1]), n


def test_params_record_is_a_float_and_an_int():
    from manhattanslam_amd import BOW_MATCH_PARAMS_DTYPE
    assert BOW_MATCH_PARAMS_DTYPE.itemsize == 8 and BOW_MATCH_PARAMS_DTYPE.names == ("nn_ratio", "check_orientation")


def test_vocab_without_a_device_fails_and_does_not_compute(tmp_path):
    """No CPU fallback: without an MI355X both constructors return NULL with an error (after checking their arguments)."""
    from manhattanslam_amd import MslError, device_count
    from manhattanslam_amd.bow import Vocabulary
    if device_count() > 0:
        pytest.skip("GPU present")
    parent = np.array([0, 0, 0], np.int32)
    with pytest.raises(MslError, match="no HIP device|no CPU fallback"):
        Vocabulary(2, 1, 0, 0, parent, np.array([0, 1, 1], np.uint8), np.zeros((3, 32), np.uint8), np.ones(3))
    p = tmp_path / "voc.txt"
    p.write_text("2 1 0 0\n0 1 " + "0 " * 32 + "1.0\n0 1 " + "1 " * 32 + "1.0\n")
    with pytest.raises(MslError, match="no HIP device|no CPU fallback"):
        Vocabulary.from_text(p)


def test_bad_vocabularies_are_refused_before_the_device():
    """Argument checks come first: a header outside the loader's limits or a parent after its child is refused on any machine."""
    from manhattanslam_amd import MslError
    from manhattanslam_amd.bow import Vocabulary
    z = np.zeros((3, 32), np.uint8)
    for k, L, sc, wt in ((1, 1, 0, 0), (21, 1, 0, 0), (2, 0, 0, 0), (2, 11, 0, 0), (2, 1, 6, 0), (2, 1, 0, 4)):
        with pytest.raises(MslError, match="invalid argument"):
            Vocabulary(k, L, sc, wt, np.array([0, 0, 0], np.int32), np.ones(3, np.uint8), z, np.ones(3))
    with pytest.raises(MslError, match="parent"):
        Vocabulary(2, 1, 0, 0, np.array([0, 2, 0], np.int32), np.ones(3, np.uint8), z, np.ones(3))

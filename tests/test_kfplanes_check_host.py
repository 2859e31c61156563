"""The index and sort checks a host-memory call of msl_keyframe_planes / msl_manhattan_observe makes
(manhattanslam_amd/csrc/msl_index_check.h), called by a plain C++ host program on exactly sized arrays (tests/kfplanes_check_host.cpp) built
with the address and undefined-behaviour sanitizers.  Runs without a GPU."""
from tests.test_mappoint_csr_host import run_sanitized


def test_kfplanes_checks_accept_valid_arrays_and_name_every_defect(tmp_path):
    run_sanitized(tmp_path, "kfplanes_check_host")

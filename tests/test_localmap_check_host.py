"""The index checks a host-memory call of msl_local_keyframes / msl_local_points / msl_local_lines makes
(manhattanslam_amd/csrc/msl_index_check.h), called by a plain C++ host program on exactly sized arrays (tests/localmap_check_host.cpp)
built with the address and undefined-behaviour sanitizers.  Runs without a GPU."""
from tests.test_mappoint_csr_host import run_sanitized


def test_local_map_checks_accept_valid_arrays_and_name_every_defect(tmp_path):
    run_sanitized(tmp_path, "localmap_check_host")

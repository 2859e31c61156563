"""The index checks a host-memory call of msl_cull_keyframes / msl_cull_recent makes (manhattanslam_amd/csrc/msl_index_check.h, the
observation table with obs_idx included), called by a plain C++ host program on exactly sized arrays
(tests/cull_check_host.cpp) built with the address and undefined-behaviour sanitizers.  Runs without a GPU."""
from tests.test_mappoint_csr_host import run_sanitized


def test_cull_checks_accept_valid_arrays_and_name_every_defect(tmp_path):
    run_sanitized(tmp_path, "cull_check_host")

"""The index checks a host-memory call of msl_observations_apply makes (manhattanslam_amd/csrc/msl_index_check.h: the observation table
through csr_ok, its ranges strictly ascending, the log's codes, fields, order and counts), called by a plain C++ host program on exactly
sized arrays (tests/observations_check_host.cpp) built with the address and undefined-behaviour sanitizers.  Runs without a GPU."""
from tests.test_mappoint_csr_host import run_sanitized


def test_observation_checks_accept_valid_arrays_and_name_every_defect(tmp_path):
    run_sanitized(tmp_path, "observations_check_host")

"""The index checks a host-memory call of msl_connections_apply and msl_fuse_targets makes (manhattanslam_amd/csrc/msl_index_check.h: the
weights, the ordered rows under a full count, the parents, the origin, the log's codes and fields, the current keyframes), called by a
plain C++ host program on exactly sized arrays (tests/connections_check_host.cpp) built with the address and undefined-behaviour
sanitizers.  Runs without a GPU."""
from tests.test_mappoint_csr_host import run_sanitized


def test_connection_checks_accept_valid_arrays_and_name_every_defect(tmp_path):
    run_sanitized(tmp_path, "connections_check_host")

"""The index checks a host-memory call of msl_plane_clouds / msl_map_plane_merge makes (manhattanslam_amd/csrc/msl_index_check.h: offsets_ok,
vertex_indices_ok, merge_into_ok), called by a plain C++ host program on exactly sized arrays (tests/plane_cloud_check_host.cpp) built with
the address and undefined-behaviour sanitizers.  Runs without a GPU."""
from tests.test_mappoint_csr_host import run_sanitized


def test_plane_cloud_checks_accept_valid_arrays_and_name_every_defect(tmp_path):
    run_sanitized(tmp_path, "plane_cloud_check_host")

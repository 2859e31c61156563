"""The index checks a host-memory call of the LocalMapping entry points makes (manhattanslam_amd/csrc/msl_index_check.h), called by plain C++
host programs on exactly sized arrays, built with the address and undefined-behaviour sanitizers: the observation table, the items and the
reference keyframes of msl_refresh_map_points / msl_covisibility (tests/mappoint_csr_host.cpp); the items and lists of msl_fuse_map_points /
msl_fuse_map_lines, the neighbours of msl_triangulate_new_points and the targets of msl_fuse_candidates (tests/mapping_lists_host.cpp).
Runs without a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_sanitized(tmp_path, name):
    exe = tmp_path / name
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                        os.path.join(ROOT, "manhattanslam_amd", "csrc"), os.path.join(ROOT, "tests", name + ".cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout + r.stderr[-3000:]


def test_csr_check_accepts_valid_tables_and_names_every_defect(tmp_path):
    run_sanitized(tmp_path, "mappoint_csr_host")


def test_list_neighbour_and_target_checks_refuse_every_defect_with_the_library_message(tmp_path):
    run_sanitized(tmp_path, "mapping_lists_host")

"""The index checks a host-memory call of msl_refresh_map_points / msl_covisibility makes (manhattanslam_amd/csrc/msl_mappoint_check.h: the
observation table, the items, the reference keyframes) called by a plain C++ host program (tests/mappoint_csr_host.cpp) on exactly sized
arrays, built with the address and undefined-behaviour sanitizers.  Runs without a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_csr_check_accepts_valid_tables_and_names_every_defect(tmp_path):
    exe = tmp_path / "mappoint_csr_host"
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                        os.path.join(ROOT, "manhattanslam_amd", "csrc"), os.path.join(ROOT, "tests", "mappoint_csr_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout + r.stderr[-3000:]

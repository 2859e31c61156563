"""The integer pieces of k_describe and k_pyramid (manhattanslam_amd/csrc/msl_orb_sums.h: IC_Angle's patch summed four pixels at a time against
weight words built from umax[]; the resize's run of four pixels from aligned source words) called by a plain C++ host program
(tests/orb_sums_host.cpp) that compares them with the literal loops, built with the address and undefined-behaviour sanitizers.  Runs without a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ic_angle_and_resize_pieces_match_literal_loops(tmp_path):
    exe = tmp_path / "orb_sums_host"
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                        os.path.join(ROOT, "manhattanslam_amd", "csrc"), os.path.join(ROOT, "tests", "orb_sums_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout + r.stderr[-3000:]

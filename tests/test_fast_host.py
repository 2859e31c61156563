"""The integer pieces of k_fast (manhattanslam_amd/csrc/msl_orb_fast.h: packed quick test of four pixels, FAST-9/16 score) called by a plain C++
host program (tests/fast_host.cpp) that compares them with a literal scalar FAST, built with the address and undefined-behaviour sanitizers.
Runs without a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fast_pieces_match_literal_fast(tmp_path):
    exe = tmp_path / "fast_host"
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                        os.path.join(ROOT, "manhattanslam_amd", "csrc"), os.path.join(ROOT, "tests", "fast_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout + r.stderr[-3000:]

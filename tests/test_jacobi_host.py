"""The pinned Jacobi eigen-solver (manhattanslam_amd/csrc/msl_jacobi.h: schedule, rotation and the register-resident sweep for n = 3 and n = 4)
called by a plain C++ host program (tests/jacobi_host.cpp) that compares it bit for bit with a literal scalar transcription of the pinned
procedure on the generic round-robin schedule, built with contraction off and the address and undefined-behaviour sanitizers.  Runs without
a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_register_solver_matches_literal_procedure(tmp_path):
    exe = tmp_path / "jacobi_host"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                        os.path.join(ROOT, "manhattanslam_amd", "csrc"), os.path.join(ROOT, "tests", "jacobi_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout + r.stderr[-3000:]

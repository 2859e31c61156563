"""The transfer planner of msl_sf_fuse_ex (manhattanslam_amd/csrc/msl_sf_plan.h: runs of touched sub-blocks, gap bridging, list-or-runs choice)
called by a plain C++ host program (tests/sf_hostvec_host.cpp) that compares it with a literal restatement of the loop the entry point used to
carry inline, built with the address and undefined-behaviour sanitizers.  Runs without a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_download_matches_the_inline_loop(tmp_path):
    exe = tmp_path / "sf_hostvec_host"
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                        os.path.join(ROOT, "manhattanslam_amd", "csrc"), os.path.join(ROOT, "tests", "sf_hostvec_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout + r.stderr[-3000:]

"""The folded pieces of k_fast (manhattanslam_amd/csrc/msl_orb_fast.h): fast_score16 with the centre value added once behind the min/max
network, and fast_quick4_at with one byte permute per 16-bit pair.  A plain C++ host program (tests/fast_fold_host.cpp) compares both with the
expressions they replace, kept verbatim in it: every centre value 0 .. 255 against 10^5 random and the structured rings; every byte alignment
0 .. 3 at thresholds 0, 7, 20, 255.  The sanitized build (address, undefined behaviour) runs the same cases with 4 000 of the random rings: it
is there for what the instrumentation sees, which does not depend on the ring count, and is ten times slower per ring.  Runs without a GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags, args", [(["-O2"], []), (["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], ["4000"])],
                         ids=["plain", "sanitized"])
def test_folded_fast_pieces_match_the_forms_before(tmp_path, flags, args):
    exe = tmp_path / "fast_fold_host"
    r = subprocess.run(["g++", "-std=c++14", *flags, "-I", os.path.join(ROOT, "manhattanslam_amd", "csrc"),
                        os.path.join(ROOT, "tests", "fast_fold_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout + r.stderr[-3000:]

"""The float / double identities of the superpixel kernels (manhattanslam_amd/csrc/msl_sf_sp_arith.h: the one-step division by 100, the fused depth
term of the cost, the Newton quotient as a float division, the comparisons with 0.01 / 0.2, the transposed 16-lane FP64 sums) called by a plain C++
host program (tests/sp_arith_host.cpp) that compares them bit for bit with the literal expressions, built with the address and undefined-behaviour
sanitizers.  Runs without a GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_superpixel_arithmetic_matches_literal_expressions(tmp_path):
    from tests import sp_arith_inputs
    exe = tmp_path / "sp_arith_host"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                        os.path.join(ROOT, "manhattanslam_amd", "csrc"), os.path.join(ROOT, "tests", "sp_arith_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout + r.stderr[-3000:]
    # the GPU test's inputs (tests/sp_arith_inputs.py) are the ones this program found sensitive to the order of the additions
    m = re.search(r"groups checksum ([0-9a-f]{16})", r.stdout)
    assert m and int(m.group(1), 16) == sp_arith_inputs.checksum(), (m and m.group(1), hex(sp_arith_inputs.checksum()))


def test_array_model_of_the_butterfly():
    """The numpy model of the row operations: totals agree in every lane, and are the exact sum where every partial sum is exact."""
    import numpy as np
    from tests import sp_arith_inputs
    v = np.arange(1, 17, dtype=np.float64)[None, :] * np.array([[1.0], [2.0 ** 30], [-3.0]])
    s = sp_arith_inputs.butterfly(v)
    assert np.array_equal(s, np.repeat(v.sum(axis=1, keepdims=True), 16, axis=1))
    x = sp_arith_inputs.group_inputs(64, 10)
    s = sp_arith_inputs.butterfly(x)
    assert np.array_equal(s.view(np.uint64), np.repeat(s[..., :1], 16, axis=-1).view(np.uint64))
    assert np.all(np.abs(np.frexp(x)[1] - 1) <= 40)

"""k_pyramid computes runs of four adjacent pixels of a row per lane: every pyramid level against the CPU oracle, byte for byte, and the fused
launch against one k_resize launch per level (MSL_ORB_PYRAMID=levels, a child process: the mode is read once per process).  Geometries where a
run can go wrong: level and tile widths that are no multiples of four, own ranges that start or end inside a run, a remainder of one pixel;
an input whose row stride exceeds its width, and a batch of three frames."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (width, height, levels, scale factor)
GEOMETRIES = ((400, 304, 6, 1.2), (641, 479, 8, 1.2), (322, 243, 8, 1.2), (640, 160, 4, 1.2), (640, 160, 3, 1.5))

CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %(root)r)
from manhattanslam_amd import ORBextractor, synth
from tests import oracle_lib
o = oracle_lib.load()
fused = %(fused)r
for (w, h, nl, sf) in %(geoms)r:
    k = max(-(-w // 640), -(-h // 480))
    img = synth.orb_frame(synth.ORB_SEED + 21 + w, 640 * k, 480 * k)[:h, :w]          # a view: its row stride is 640 k >= w
    ex = ORBextractor(300, sf, nl, 20, 7, max_width=w, max_height=h, max_batch=3)
    ex.profile_enable()
    kg, dg = ex(img)
    launches = ex.profile_read()["k_pyramid"][1]
    assert launches == (1 if fused else nl - 1), (w, h, launches)          # the fused kernel really ran (or, per level, really did not)
    ex.profile_enable(0)
    oe = o.orb_create(300, sf, nl, 20, 7)
    ko, do = oe.extract(np.ascontiguousarray(img))
    for l in range(1, nl):
        assert np.array_equal(ex.debug_level(0, l), oe.level(l)), (w, h, l)
    assert kg.tobytes() == ko.tobytes() and np.array_equal(dg, do), (w, h)
    if (w, h, nl) == (322, 243, 8):          # a batch of three different frames: every frame's levels
        imgs = np.stack([np.ascontiguousarray(img), synth.orb_frame(5, w, h), np.ascontiguousarray(img[::-1])])
        res = ex.extract_batch(imgs)
        for f in (2, 1, 0):
            ko, do = oe.extract(imgs[f])          # (the oracle keeps the levels of its last frame)
            for l in range(1, nl):
                assert np.array_equal(ex.debug_level(f, l), oe.level(l)), ("batch", f, l)
            assert res[f][0].tobytes() == ko.tobytes() and np.array_equal(res[f][1], do), ("batch", f)
    ex.close()
print("pyramid runs ok")
"""


@pytest.mark.parametrize("mode", ["fused", "levels"])
def test_pyramid_levels_match_oracle(mode):
    script = CHILD % dict(root=ROOT, fused=mode == "fused", geoms=GEOMETRIES)
    env = dict(os.environ, MSL_ORB_PYRAMID=mode)
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "pyramid runs ok" in r.stdout, mode + "\n" + r.stdout + r.stderr[-3000:]

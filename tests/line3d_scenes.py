"""Fixed scenes for msl_lines_3d: small synthetic depth images (160 x 120 unless stated) with keylines chosen for the places the kernel can go
wrong.  scene(name) -> dict(line_ends, depth, Tcw, seed, line_flags, what); model(name, order) -> the sequential model's frame result
(tests/line3d_model.py), computed once and shared.  Seeds are chosen so that tests/test_line3d_model.py::test_margins holds."""
import functools
import math

import numpy as np

from tests import line3d_model as lm

W, H = 160, 120
F32 = np.float32
PARAMS = lm.default_params(fx=100.0, fy=100.0, cx=79.5, cy=59.5)
BIG_PARAMS = lm.default_params(fx=525.0, fy=525.0, cx=319.5, cy=239.5)


def pose(seed):
    """A camera pose: rows 0-2 of a CV_32F Tcw."""
    r = np.random.RandomState(seed)
    w = r.uniform(-0.3, 0.3, 3)
    th = np.linalg.norm(w); k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K
    return np.concatenate([R, r.uniform(-1, 1, (3, 1))], 1).astype(F32)


def plane(w=W, h=H, z0=1.5, gu=0.004, gv=0.003):
    """A tilted plane seen as a depth image, noiseless."""
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    return (z0 + gu * u + gv * v).astype(F32)


def _hline(x0, y, length):
    return [x0, y, x0 + length, y]


def _keep_only(depth, ends, keep, prm=PARAMS):
    """Zeroes the depth under every sample of the keyline for which keep(k, n) is false (k: position among the n samples inside the image)."""
    _, pix = lm.sample_pixels(ends, depth.shape, prm)
    for k, (r, c) in enumerate(pix):
        if not keep(k, len(pix)):
            depth[r, c] = 0.0


def _scene(ends, depth, seed, what, flags=None):
    ends = np.asarray(ends, F32).reshape(-1, 4)
    n = len(ends)
    return dict(line_ends=ends, depth=np.ascontiguousarray(depth, F32), Tcw=pose(seed), seed=(np.arange(n, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(seed)),
                line_flags=np.zeros(n, np.uint8) if flags is None else np.asarray(flags, np.uint8), what=what)


def _short():
    return _scene([_hline(20.3, 30.2 + 7 * i, L) for i, L in enumerate((0.5, 8.5, 9.5, 10.5))], plane(), 11, "(int)len = 0, 8, 9, 10: 9 is the first that can succeed")


def _wave():
    return _scene([[10.3, 20.2 + 9 * i, 10.3 + L, 24.9 + 9 * i] for i, L in enumerate((62.3, 63.3, 64.3))], plane(), 12, "63, 64 and 65 kept samples")


def _holes():
    d = plane()
    ends = [_hline(10.5, 40.5, 20.5), _hline(10.5, 60.5, 20.5), [30.2, 80.1, 70.9, 95.3]]
    _keep_only(d, ends[0], lambda k, n: k % 2 == 0 and k not in (10, 12))    # 9 of 21 (both end points keep their depths)
    _keep_only(d, ends[1], lambda k, n: k % 2 == 0 and k != 10)              # 10 of 21, spread over nine cells
    _keep_only(d, ends[2], lambda k, n: k not in (1, 5, 17))
    return _scene(ends, d, 13, "depth holes that leave 9 and 10 samples; scattered holes")


def _integer():
    return _scene([[10, 20, 50, 20], [30, 40, 30, 90], [0, 0, 30, 40], [12, 100, 72, 100.5]], plane(), 14,
                  "axis-aligned keylines with integral end points: the integer-coordinate quirk, also at column / row 0")


def _outside():
    ends = [[-0.7, 30.2, 60.4, 50.1], [20.3, -0.4, 90.2, 40.7], [100.2, 20.3, 159.6, 70.8], [100.2, 60.3, 170.0, 70.8], [30.5, 100.2, 80.3, 120.0],
            [-1.0, 50.5, 40.0, 50.5], [159.9, 119.9, 110.2, 80.4]]
    return _scene(ends, plane(), 15, "end points that truncate into the image (-0.7 -> 0) with samples outside, and end points outside it")


def _step():
    d = plane()
    d[:, 64:] += F32(1.0)
    return _scene([[20.4, 30.3, 130.2, 36.8], [140.3, 70.2, 25.1, 66.4], [30.2, 90.3, 120.4, 90.9]], d, 16, "keylines across a depth step: two structures")


def _cells():
    d = plane()
    ends = [_hline(20.5, 30.5, 50.3), _hline(20.5, 50.5, 50.3)]
    _keep_only(d, ends[0], lambda k, n: not (0.32 * n < k < 0.66 * n))       # cells 3, 4, 5 empty: seven of ten
    _keep_only(d, ends[1], lambda k, n: not (0.32 * n < k < 0.56 * n))       # cells 3, 4 empty: eight of ten
    return _scene(ends, d, 17, "samples bunched into seven / eight of verify3dLine's ten cells")


def _accept():
    d = plane()
    ends = [_hline(20.5, 20.5, 50.3), _hline(20.5, 35.5, 50.3), _hline(20.5, 60.5, 9.4), _hline(20.5, 80.5, 9.4)]
    _keep_only(d, ends[0], lambda k, n: k < 20)                             # 20 / 50.3 < 0.4
    _keep_only(d, ends[1], lambda k, n: k < 21 or k == n - 1)               # enough support; the far end point keeps its depth
    d[20, 70] = plane()[20, 70]
    d[56:66, :] = F32(0.2)                                                   # 9 pixels of 2 mm: below min_length
    d[76:86, :] = F32(0.25)                                                  # 9 pixels of 2.5 mm: above
    return _scene(ends, d, 18, "support ratio and 3-D length on either side of their thresholds")


def _sigma_zero():
    d = plane()
    d[30:40, :] = F32(0.34538)                                               # sigma(z) ~ 0: inverse square roots go infinite
    d[50:60, 40:44] = F32(0.34538)
    return _scene([_hline(20.5, 35.5, 31.4), _hline(20.5, 55.5, 40.4)], d, 19, "sample depths near 0.345 m: non-finite DU, NaN distances")


def _noisy(seed, n=12, sigma=1.2, w=W, h=H, prm=PARAMS, min_len=12.0, max_len=90.0):
    r = np.random.RandomState(seed)
    d = plane(w, h).astype(np.float64)
    d = d + sigma * lm.depth_std_dev(d) * r.standard_normal(d.shape)
    ends = []
    while len(ends) < n:
        a = r.uniform([1, 1], [w - 1, h - 1]); b = r.uniform([1, 1], [w - 1, h - 1])
        if min_len <= np.linalg.norm(a - b) <= max_len:
            ends.append([a[0], a[1], b[0], b[1]])
    return np.array(ends, F32), d.astype(F32)


def _refit():
    ends, d = _noisy(21, n=10, sigma=1.0)
    return _scene(ends, d, 21, "depth noise: the refit loop runs more than one round")


def _one():
    return _scene([[20.4, 30.3, 70.2, 56.8]], plane(), 22, "n_lines = 1")


def _none():
    return _scene(np.zeros((0, 4), F32), plane(), 23, "n_lines = 0")


def _full():
    ends, d = _noisy(24, n=256, sigma=0.8, min_len=10.0, max_len=22.0)
    r = np.random.RandomState(5)
    flags = r.choice([0, 1, 3], 256, p=[0.7, 0.1, 0.2]).astype(np.uint8)
    d[r.randint(0, H, 300), r.randint(0, W, 300)] = 0.0
    return _scene(ends, d, 24, "lcap = 256 full, held keylines, more than max_new_lines successes: the 31st-line stop", flags)


def _big():
    d = plane(640, 480, 1.2, 0.001, 0.0008)
    ends = [[50.3, 60.2, 150.3 + 0.4, 60.9], [30.2, 100.4, 280.1, 100.9], [600.2, 20.3, 350.4, 470.2], [10.4, 400.3, 630.2, 410.9], [300.5, 200.5, 309.9, 200.5]]
    return _scene(ends, d, 25, "one 640 x 480 frame: len 100 and 250 and beyond, the max_samples cap gives 101 samples")


_BUILD = dict(short=_short, wave=_wave, holes=_holes, integer=_integer, outside=_outside, step=_step, cells=_cells, accept=_accept,
              sigma_zero=_sigma_zero, refit=_refit, one=_one, none=_none, full=_full, big=_big)
SMALL = ("short", "wave", "holes", "integer", "outside", "step", "cells", "accept", "sigma_zero", "refit", "one", "none")   # one ragged batch
ALL_SCENES = SMALL + ("full", "big")


def params(name):
    return BIG_PARAMS if name == "big" else PARAMS


@functools.lru_cache(maxsize=None)
def scene(name):
    return _BUILD[name]()


_CACHE = {}


@functools.lru_cache(maxsize=None)
def model(name, order=lm.ALL):
    """The model's result for the scene as one frame; the per-keyline results are shared between the orders (treat as read-only)."""
    s = scene(name)
    # the ordered modes skip keylines held with observations, which ALL computes: one cache serves both because a result is per keyline
    return lm.lines_3d(order, params(name), s["line_ends"], s["depth"], s["line_flags"], s["Tcw"], s["seed"], cache=_CACHE.setdefault(name, {}))

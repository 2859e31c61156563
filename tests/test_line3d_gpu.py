"""msl_lines_3d on the device against its sequential model (tests/line3d_model.py) on the fixed scenes of tests/line3d_scenes.py: every output
identical -- line_xyz as bytes --, the debug accessor's draws, counts, records, refit rounds and end-point indices identical, and its m, d
bit-identical (the kernel runs the model's operations in the model's order; tests/test_line3d_model.py::test_margins keeps every decision
away from its threshold all the same)."""
import numpy as np
import pytest

from tests import line3d_model as lm
from tests import line3d_scenes as ls

pytestmark = pytest.mark.gpu
ORDERS = (lm.ALL, lm.INDEX_ORDER, lm.DEPTH_ORDER)
KEYS = ("line_depth", "line_xyz", "line_ok", "line_new", "n_support", "n_new")


def _params(p):
    from manhattanslam_amd import line3d
    return line3d.line3d_params(**p)


@pytest.fixture(scope="module")
def matcher():
    from manhattanslam_amd.match import Matcher
    h = Matcher()
    yield h
    h.close()


def _run(names, order, handle=None, lcap=None):
    from manhattanslam_amd import line3d
    return line3d.lines_3d(_params(ls.params(names[0])), [ls.scene(n) for n in names], order, handle=handle, lcap=lcap)


def _check(names, order, got):
    lcap = got["line_ok"].shape[1]
    for f, name in enumerate(names):
        m = ls.model(name, order)
        n = len(m["line_ok"])
        for k in ("line_depth", "line_xyz", "line_ok", "line_new", "n_support"):
            assert got[k][f, :n].tobytes() == m[k].tobytes(), (name, order, k, got[k][f, :n], m[k])
        assert int(got["n_new"][f]) == m["n_new"], (name, order)
        # beyond n_lines: no depth, no line
        assert np.all(got["line_depth"][f, n:] == -1) and not got["line_xyz"][f, n:].any() and not got["line_ok"][f, n:].any()
        assert not got["line_new"][f, n:].any() and not got["n_support"][f, n:].any() and n <= lcap


def _check_debug(names, order, handle):
    from manhattanslam_amd import line3d
    same = total = 0
    for f, name in enumerate(names):
        m = ls.model(name, order)
        for j, r in enumerate(m["lines"]):
            d = line3d.debug_lines(handle, f, j)
            if r is None:
                assert d["n_kept"] == 0 and not d["iters"] and d["refits"] == 0
                continue
            t = r["trace"]
            assert d["n_kept"] == r["n_kept"], (name, j, d["n_kept"], r["n_kept"])
            assert d["iters"] == [tuple(x) for x in t["iters"]], (name, j, d["iters"], t["iters"])
            assert d["refits"] == t["refits"] and d["ends"] == tuple(t["ends"]), (name, j, d, t["refits"], t["ends"])
            total += 1
            same += d["m"].tobytes() == np.array(t["m"]).tobytes() and d["d"].tobytes() == np.array(t["d"]).tobytes()
            assert d["m"].tobytes() == np.array(t["m"]).tobytes() and d["d"].tobytes() == np.array(t["d"]).tobytes(), (name, j, d["m"], t["m"], d["d"], t["d"])
    print("keylines with bit-identical m, d:", same, "of", total)


@pytest.mark.parametrize("order", ORDERS)
def test_ragged_batch_matches_model(matcher, order):
    """Twelve 160 x 120 frames of different n_lines (0 and 1 among them) in one call: outputs and the per-keyline stage."""
    got = _run(ls.SMALL, order, handle=matcher)
    _check(ls.SMALL, order, got)
    _check_debug(ls.SMALL, order, matcher)


@pytest.mark.parametrize("order", ORDERS)
def test_full_capacity(matcher, order):
    """lcap = 256 with every slot used, held keylines, and more successes than max_new_lines: the walk's stop."""
    got = _run(("full",), order, handle=matcher)
    assert got["line_ok"].shape[1] == 256
    _check(("full",), order, got)
    m = ls.model("full", order)
    if order != lm.ALL:
        assert m["n_new"] < int(m["line_ok"].sum()) and m["n_new"] <= 31          # the stop cut the walk short


def test_big_frame(matcher):
    """One 640 x 480 frame: len 100 and 250 and beyond, where the max_samples cap gives 101 samples."""
    got = _run(("big",), lm.DEPTH_ORDER, handle=matcher)
    _check(("big",), lm.DEPTH_ORDER, got)
    _check_debug(("big",), lm.DEPTH_ORDER, matcher)
    assert [r["n_kept"] for r in ls.model("big", lm.DEPTH_ORDER)["lines"][:4]] == [101] * 4


def test_memory_spaces_and_batch_form(matcher):
    """Host memory, device memory (asynchronous on the handle's stream) and the device-indexed form give the same bytes."""
    import torch
    from manhattanslam_amd import line3d
    names = ls.SMALL
    prm = _params(ls.params(names[0]))
    frames = [ls.scene(n) for n in names]
    host = line3d.lines_3d(prm, frames, lm.DEPTH_ORDER, handle=matcher)
    batch = line3d.lines_3d(prm, frames, lm.DEPTH_ORDER)
    lcap, W, H, a = line3d.pack_lines(frames)
    B = len(frames)
    dev = {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).cuda() for k, v in a.items()}
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    out = dict(line_depth=z((B, lcap, 2), torch.float32), line_xyz=z((B, lcap, 6), torch.float64), line_ok=z((B, lcap), torch.uint8),
               line_new=z((B, lcap), torch.uint8), n_support=z((B, lcap), torch.int32), n_new=z(B, torch.int32))
    torch.cuda.synchronize()
    line3d.lines_3d_device(matcher, prm, B, lcap, lm.DEPTH_ORDER, dev["line_ends"], dev["n_lines"], dev["depth"], 4 * W, 4 * W * H, W, H,
                           dev["line_flags"], dev["Tcw"], dev["seed"], *[out[k] for k in KEYS])
    matcher.sync()
    for k in KEYS:
        assert out[k].cpu().numpy().tobytes() == host[k].tobytes(), k
        assert batch[k].tobytes() == host[k].tobytes(), k
    # a NULL line_flags is all zeros
    none = {k: np.zeros_like(host[k]) for k in KEYS}
    from manhattanslam_amd._lib import check, lib, ptr
    check(lib.msl_lines_3d(matcher.h, B, lcap, lm.DEPTH_ORDER, ptr(prm), ptr(a["line_ends"]), ptr(a["n_lines"]), ptr(a["depth"]), 4 * W, 4 * W * H, W, H,
                           None, ptr(a["Tcw"]), ptr(a["seed"]), 0, *[ptr(none[k]) for k in KEYS], 0))
    for k in KEYS:
        assert none[k].tobytes() == host[k].tobytes(), k


def test_handle_growth_and_padded_rows():
    """A small call, then a larger lcap and more frames on the same handle (its scratch grows), then the small one again: each equals the
    model; a depth image with padded rows and a padded frame stride reads the same pixels."""
    from manhattanslam_amd import line3d
    from manhattanslam_amd._lib import check, lib, ptr
    from manhattanslam_amd.match import Matcher
    h = Matcher()
    small = ("one", "short")
    _check(small, lm.INDEX_ORDER, _run(small, lm.INDEX_ORDER, handle=h))
    _check_debug(small, lm.INDEX_ORDER, h)
    large = ("refit", "step", "wave", "one", "holes")
    _check(large, lm.INDEX_ORDER, _run(large, lm.INDEX_ORDER, handle=h, lcap=64))
    _check_debug(large, lm.INDEX_ORDER, h)
    got = _run(small, lm.INDEX_ORDER, handle=h)
    _check(small, lm.INDEX_ORDER, got)
    prm = _params(ls.params("one"))
    lcap, W, H, a = line3d.pack_lines([ls.scene(n) for n in small])
    padded = np.full((2, H + 3, W + 5), 7.0, np.float32)
    padded[:, :H, :W] = a["depth"]
    out = {k: np.zeros_like(got[k]) for k in KEYS}
    check(lib.msl_lines_3d(h.h, 2, lcap, lm.INDEX_ORDER, ptr(prm), ptr(a["line_ends"]), ptr(a["n_lines"]), ptr(padded), 4 * (W + 5), 4 * (W + 5) * (H + 3),
                           W, H, ptr(a["line_flags"]), ptr(a["Tcw"]), ptr(a["seed"]), 0, *[ptr(out[k]) for k in KEYS], 0))
    for k in KEYS:
        assert out[k].tobytes() == got[k].tobytes(), k
    h.close()


def test_refusals(matcher):
    """Every limit: MSL_ERR_INVALID with msl_last_error() naming the field, before any launch -- the outputs keep their bytes (both forms)."""
    from manhattanslam_amd import line3d
    from manhattanslam_amd._lib import lib, ptr
    frames = [ls.scene("one")]
    _, W, H, a = line3d.pack_lines(frames, lcap=257)
    p0 = dict(ls.params("one"))

    def call(batch, lcap=1, order=lm.ALL, row=4 * W, frame=4 * W * H, n_frames=1, **kw):
        prm = _params(dict(p0, **kw))
        out = dict(line_depth=np.full((257, 2), 3, np.float32), line_xyz=np.full((257, 6), 3, np.float64), line_ok=np.full(257, 3, np.uint8),
                   line_new=np.full(257, 3, np.uint8), n_support=np.full(257, 3, np.int32), n_new=np.full(1, 3, np.int32))
        args = (n_frames, lcap, order, ptr(prm), ptr(a["line_ends"]), ptr(a["n_lines"]), ptr(a["depth"]), row, frame, W, H, ptr(a["line_flags"]),
                ptr(a["Tcw"]), ptr(a["seed"]), 0, *[ptr(out[k]) for k in KEYS], 0)
        rc = lib.msl_lines_3d_batch(0, *args) if batch else lib.msl_lines_3d(matcher.h, *args)
        return rc, lib.msl_last_error().decode(), all(np.all(v == 3) for v in out.values())

    for batch in (False, True):
        for kw, field in ((dict(lcap=257), "lcap"), (dict(lcap=0), "lcap"), (dict(max_samples=128), "max_samples"), (dict(max_samples=0), "max_samples"),
                          (dict(max_iterations=65), "max_iterations"), (dict(max_iterations=-1), "max_iterations"), (dict(min_points=1), "min_points"),
                          (dict(order=3), "order"), (dict(order=-1), "order"), (dict(row=4 * W - 4), "strides"), (dict(row=4 * W + 2), "strides"),
                          (dict(n_frames=0), "n_frames")):
            rc, msg, untouched = call(batch, **kw)
            assert rc == -1 and field in msg and untouched, (batch, kw, rc, msg, untouched)
        rc, _, untouched = call(batch, lcap=256, max_samples=127, max_iterations=64, min_points=2)      # the limits themselves are accepted
        assert rc == 0 and not untouched


def _chain_frames(B=2, n_kl=20, lcap=32):
    """Frame t: keylines over a noiseless tilted plane (640 x 480) under a random pose.  Frame t + 1: the camera a little further on; its
    keylines are the projections of frame t's lines (the model's) with pixel noise, its descriptors noisy copies."""
    from tests import line_match_scenes as lsc
    pll = lsc.params(15.0)
    prm = lm.default_params(*(float(pll[k][0]) for k in ("fx", "fy", "cx", "cy")))
    depth = ls.plane(640, 480, 1.2, 0.001, 0.0008)
    t_frames, models, cur, last, Tc, Tl = [], [], [], [], [], []
    for f in range(B):
        rng = np.random.Generator(np.random.PCG64(700 + f))
        ends = []
        while len(ends) < n_kl:
            a, b = rng.uniform([5, 5], [635, 475]), rng.uniform([5, 5], [635, 475])
            if 40 <= np.linalg.norm(a - b) <= 200:
                ends.append([a[0], a[1], b[0], b[1]])
        T = lsc.pose(rng)
        fr = dict(line_ends=np.array(ends, np.float32), depth=depth, Tcw=T[:3, :4].copy(), seed=rng.integers(0, 2 ** 32, n_kl, dtype=np.uint32))
        m = lm.lines_3d(lm.DEPTH_ORDER, prm, fr["line_ends"], depth, None, fr["Tcw"], fr["seed"])
        T1 = T.copy(); T1[:3, 3] += np.array([0.03, -0.02, 0.05], np.float32)
        base = rng.integers(0, 256, (n_kl, 32), dtype=np.uint8)
        xy1 = rng.uniform(20, 620, (n_kl, 2)); xy2 = rng.uniform(20, 460, (n_kl, 2))
        desc = rng.integers(0, 256, (n_kl, 32), dtype=np.uint8); slope = np.zeros(n_kl)
        for i in range(n_kl):
            q = lsc._project(pll, T1, m["line_xyz"][i]) if m["line_ok"][i] else None
            if q is not None and np.all(np.isfinite(q)):
                xy1[i] = q[:2] + rng.normal(0, 0.3, 2); xy2[i] = q[2:] + rng.normal(0, 0.3, 2)
                desc[i] = lsc.desc_flip(rng, base[i], int(rng.integers(0, 30)))
                slope[i] = (q[1] - q[3]) / (q[0] - q[2]) if q[0] != q[2] else 0.0
        octave = rng.integers(0, 4, n_kl)
        cur.append(dict(kl=lsc.keylines(xy1, xy2, octave, (slope + rng.uniform(-0.05, 0.2, n_kl)).astype(np.float32)), desc=desc,
                        ends=np.concatenate([xy1, xy2], 1)))
        last.append(dict(xyz=m["line_xyz"], desc=base, flags=m["line_ok"], octave=octave.astype(np.int32)))
        t_frames.append(fr); models.append(m); Tc.append(T1); Tl.append(T)
    return pll, prm, t_frames, models, cur, last, np.stack(Tc), np.stack(Tl)


def test_chain_lines_match_pose():
    """msl_lines_3d on frame t, its line_xyz / line_ok fed as last_line_xyz / last_line_flags into msl_match_lines_by_projection for frame
    t + 1, whose line_xyz / line_has go into msl_pose_optimize: one handle, one stream, device tensors throughout, no host copy and no
    element-wise step in between.  Compared with the three models run in sequence."""
    import torch
    from manhattanslam_amd import KEYLINE_DTYPE, line3d, match, pose
    from manhattanslam_amd.match import Matcher
    from tests import line_match_model as lmm
    from tests import pose_scenes as ps
    from tests.test_line_match_gpu import _line_fn
    from tests.test_pose_gpu import _check as check_pose
    B, lcap = 2, 32
    pll, prm, t_frames, models, cur, last, Tc, Tl = _chain_frames(B, 20, lcap)
    c = ps.params(); c.update(fx=float(pll["fx"][0]), fy=float(pll["fy"][0]), cx=float(pll["cx"][0]), cy=float(pll["cy"][0]), bf=float(pll["bf"][0]))
    _, W, H, a = line3d.pack_lines(t_frames, lcap)
    _, llcap, larr = match.pack_lines_last(cur, last, Tc, Tl, lcap=lcap, llcap=lcap)
    rngp = np.random.default_rng(9)
    Tin = np.zeros((B, 12), np.float32)
    line_fn = np.zeros((B, lcap, 3))
    for f in range(B):
        R0 = ps.rot(rngp.normal(size=3), 0.5) @ Tc[f][:3, :3].astype(np.float64)
        Tin[f] = ps.tcw12(R0, Tc[f][:3, 3] + rngp.normal(size=3) * 0.01)
        line_fn[f, :len(cur[f]["kl"])] = _line_fn(cur[f]["ends"])
    h = Matcher()
    stream = torch.cuda.Stream()
    h.set_stream(stream.cuda_stream)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v.view(np.uint8) if v.dtype == KEYLINE_DTYPE else (v.view(np.int32) if v.dtype == np.uint32 else v))).cuda()
    with torch.cuda.stream(stream):
        d = {k: dev(v) for k, v in a.items()}
        o3 = dict(line_depth=z((B, lcap, 2), torch.float32), line_xyz=z((B, lcap, 6), torch.float64), line_ok=z((B, lcap), torch.uint8),
                  line_new=z((B, lcap), torch.uint8), n_support=z((B, lcap), torch.int32), n_new=z(B, torch.int32))
        dl = [dev(v) for v in larr]
        lmo = torch.full((B, lcap), -7, dtype=torch.int32, device="cuda"); lnm = z(B, torch.int32)
        cxyz, chas = z((B, lcap, 6), torch.float64), z((B, lcap), torch.uint8)
        cap = pcap = 1
        inputs = [z((B, cap, 28), torch.uint8), z((B, cap, 2), torch.float32), z((B, cap), torch.float32), z((B, cap), torch.int32), z(B, torch.int32),
                  z((B, cap, 3), torch.float32), dev(line_fn), cxyz, chas, dl[2], z((B, pcap, 4), torch.float32), z((B, pcap, 12), torch.float32),
                  z((B, pcap), torch.uint8), z(B, torch.int32), dev(Tin)]
        io = [z((B, cap), torch.uint8), z((B, lcap), torch.uint8), z((B, pcap, 3), torch.uint8)]
        Tout, ng = z((B, 12), torch.float32), z(B, torch.int32)
        stream.synchronize()                                               # the uploads and fills are done; from here on only the handle enqueues
        line3d.lines_3d_device(h, line3d.line3d_params(**prm), B, lcap, lm.DEPTH_ORDER, d["line_ends"], d["n_lines"], d["depth"], 4 * W, 4 * W * H, W, H,
                               d["line_flags"], d["Tcw"], d["seed"], *[o3[k] for k in KEYS])
        h.search_lines_by_projection_device(pll, B, lcap, llcap, dl[:3] + [o3["line_xyz"], dl[4], o3["line_ok"]] + dl[6:], lmo, lnm, cxyz, chas)
        pose.pose_optimization_device(h, pose.pose_params(c), B, (cap, cap, lcap, pcap), inputs, io, Tout, ng)
        h.sync()
    host = lambda t: t.cpu().numpy()
    # stage 1 against its model
    for f in range(B):
        n = len(models[f]["line_ok"])
        for k in ("line_depth", "line_xyz", "line_ok", "line_new", "n_support"):
            assert host(o3[k])[f, :n].tobytes() == models[f][k].tobytes(), (f, k)
        assert int(o3["n_new"][f]) == models[f]["n_new"] and models[f]["n_new"] >= 15
    # stage 2 against its model fed stage 1's output
    lx, lh, mo = host(cxyz), host(chas), host(lmo)
    model_frames, got = [], []
    for f in range(B):
        nl = len(cur[f]["kl"])
        wm, wnm = lmm.search_lines_by_projection(pll, cur[f], last[f], Tc[f], Tl[f])
        assert int(lnm[f]) == wnm and np.array_equal(mo[f, :nl], wm) and wnm >= 10, (f, int(lnm[f]), wnm)
        wx, wh = lmm.pose_layout(wm, last[f]["xyz"], lcap, np.zeros((lcap, 6)), np.zeros(lcap, np.uint8), clear=True)
        assert lx[f].tobytes() == wx.tobytes() and np.array_equal(lh[f], wh)
        # stage 3 against its model fed stage 2's output
        fr = ps.empty(0, nl, 0, cap)
        fr.update(line_fn=line_fn[f, :nl], line_xyz=lx[f, :nl], line_has=lh[f, :nl], Tcw=Tin[f])
        ps.check_margin(fr, c)
        model_frames.append(fr)
        got.append((int(ng[f]), host(Tout)[f], dict(outlier=np.zeros(0, np.uint8), line_outlier=host(io[1])[f, :nl], plane_outlier=np.zeros(0, np.uint8),
                                                  par_outlier=np.zeros(0, np.uint8), ver_outlier=np.zeros(0, np.uint8))))
    check_pose(c, model_frames, got)
    h.close()

"""GPU parity at the limits include/msl.h accepts for the tracking calls: 16-level pyramids (and 1- and 12-level ones), the top ends of
cap / mcap / mlcap / lcap / llcap / xcap / pcap, out-of-range octaves and point references, poisoned tails and unused table entries, and
batches wider than the device has CUs.  Every comparison is the one the per-call suites make: match vectors, counts, in_view, track
records, line_xyz / line_has and outlier bytes bit for bit; Tcw_out within 1e-6 (1e-5 with plane edges)."""
import numpy as np
import pytest

from tests import line_match_model as lmm
from tests import line_match_scenes as lsc
from tests import local_match_model as lm
from tests import local_match_scenes as ls
from tests import match_scenes as ms
from tests import pose_model as pm
from tests import pose_scenes as ps
from tests import translation_model as tm
from tests import translation_scenes as ts

pytestmark = pytest.mark.gpu

BAD_OCTAVES = [-1, 16, 99, 1000, -2 ** 31]


# ---- checks shared by the tests --------------------------------------------------------------------------------------------------------
def _check_points(p, cur, last, Tc, Tl, match, nm):
    from tests import oracle_lib
    tot = 0
    for f in range(len(cur)):
        want, n = oracle_lib.search_by_projection(p, cur[f], last[f], Tc[f], Tl[f])
        assert nm[f] == n and np.array_equal(match[f][:len(want)], want), (f, nm[f], n, np.flatnonzero(match[f][:len(want)] != want)[:10])
        tot += n
    return tot


def _check_local(p, cur, local, T, got):
    match, ntm, nm, inv, trk = got
    tot = 0
    for f in range(len(cur)):
        wm, wntm, wnm, winv, wtrk = lm.search_local_points(p, cur[f], local[f], T[f])
        assert ntm[f] == wntm and nm[f] == wnm, (f, ntm[f], wntm, nm[f], wnm)
        assert np.array_equal(match[f], wm), (f, np.flatnonzero(match[f] != wm)[:10])
        assert np.array_equal(inv[f], winv) and trk[f].tobytes() == wtrk.tobytes(), f
        tot += wnm
    return tot


def _check_pose(c, frames, got, model=pm.pose_optimization, rcw=None, planes=("plane", "par", "ver")):
    for f, fr in enumerate(frames):
        wn, wT, wout = model(fr, c) if rcw is None else model(fr, c, rcw[f])
        n, T, out = got[f]
        assert n == wn, (f, n, wn)
        for k, v in wout.items():
            assert np.array_equal(out[k], v), (f, k, np.flatnonzero(out[k] != v)[:10])
        tol = 1e-5 if any(np.any(fr[k + "_has"]) for k in planes) and wn != 0 else 1e-6
        assert np.max(np.abs(T.astype(np.float64) - wT)) <= tol, (f, T, wT)


def _init_io(B, lcap, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(B, lcap, 6)), rng.integers(0, 2, (B, lcap)).astype(np.uint8)


# ---- 1. last-frame point matching at cap = 8192 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlevels", [16, 1])
def test_last_frame_points_at_cap_8192(oracle, nlevels):
    """8192 keypoints and 8192 last-frame points per pair, no motion / forward / backward, check_orientation on.  At 16 levels of 1.2 the
    radius reaches 15 * 1.2^15 px, so windows hold hundreds of candidates (k_match_candidates keeps the best 32, k_match_assign's
    3 * 4 * cap LDS tables are 96 KiB); at 1 level every window is level 0.  The last frame carries octaves -1, nlevels, 15, 16 and 1000:
    outside [0, nlevels) they find no candidates (msl_match.hip's nlevels guard)."""
    from manhattanslam_amd import match, MATCH_PARAMS_DTYPE
    p = ms.params(None, 15, True, dtype=MATCH_PARAMS_DTYPE, nlevels=nlevels)
    cur, last, Tc, Tl = [], [], [], []
    for j, tz in enumerate((0.0, 0.3, -0.3)):
        c, l, a, b = ms.random_pair(1100 + 10 * nlevels + j, p, n_cur=8192, n_last=8192, tz=tz, cluster=(j == 2))
        l["octave"][j::97] = np.resize([-1, nlevels, 15, 16, 1000], len(l["octave"][j::97]))
        cur.append(c); last.append(l); Tc.append(a); Tl.append(b)
    got, nm = match.search_by_projection_batch(p, cur, last, np.stack(Tc), np.stack(Tl))
    assert _check_points(p, cur, last, Tc, Tl, got, nm) > 3000


# ---- 2. local point matching at cap 8192 / mcap 32768 / 16 levels ----------------------------------------------------------------------
def test_local_points_at_cap_8192_mcap_32768():
    """One frame at the top end (8192 keypoints, 32768 local points, predicted levels 0-15), one with 60 % pre-held keypoints and one where
    every point competes for 40 keypoints (the min-fixpoint runs many rounds at full width).  k_local_assign's LDS is int t[cap] |
    short pick[mcap] = 96 KiB here and its 16-bit item keys reach their last values."""
    from manhattanslam_amd import match
    p = ls.params(3.0, nlevels=16)
    specs = [dict(seed=1201, n_cur=8192, n_local=32768), dict(seed=1202, n_cur=4000, n_local=16000, preheld=0.6),
             dict(seed=1203, n_cur=2000, n_local=8000, conflict=True)]
    cur, local, T = [], [], []
    for s in specs:
        c, l, t = ls.random_frame(p=p, **s)
        cur.append(c); local.append(l); T.append(t)
    got = match.search_local_points_batch(p, cur, local, np.stack(T), cap=8192, mcap=32768)
    assert _check_local(p, cur, local, T, got) > 5000
    levels = got[4][0]["scale_level"][got[3][0] > 0]
    assert set(np.unique(levels)) == set(range(16))


# ---- 3. line matching at lcap = llcap = 256 and mlcap = 32768 ---------------------------------------------------------------------------
def test_last_frame_lines_at_256():
    """256 keylines and 256 last-frame lines per frame, 16 levels, keyline and last-line octaves across 0-15 plus -1, 16 and 99 (the last
    line's octave is clamped for the mvScaleFactors lookup)."""
    from manhattanslam_amd import match
    p = lsc.params(15.0, nlevels=16)
    cur, last, Tc, Tl = [], [], [], []
    for j, fwd in enumerate((0.0, 0.4, -0.4)):
        c, l, a, b = lsc.frame_pair(1300 + j, p, n_kl=256, n_last=256, octaves=16, fwd=fwd)
        c["kl"]["octave"][j::23] = np.resize([-1, 16, 99], len(c["kl"]["octave"][j::23]))
        l["octave"][j + 5::19] = np.resize([99, -1, 16], len(l["octave"][j + 5::19]))
        cur.append(c); last.append(l); Tc.append(a); Tl.append(b)
    init = _init_io(3, 256, 13)
    match_, nm, lx, lh = match.search_lines_by_projection_batch(p, cur, last, np.stack(Tc), np.stack(Tl), lcap=256, llcap=256,
                                                                line_xyz=init[0], line_has=init[1])
    tot = 0
    for f in range(3):
        wm, wnm = lmm.search_lines_by_projection(p, cur[f], last[f], Tc[f], Tl[f])
        assert nm[f] == wnm and np.array_equal(match_[f], wm), (f, nm[f], wnm, np.flatnonzero(match_[f] != wm)[:10])
        wx, wh = lmm.pose_layout(wm, last[f]["xyz"], 256, init[0][f], init[1][f], clear=True)
        assert lx[f].tobytes() == wx.tobytes() and np.array_equal(lh[f], wh), f
        tot += wnm
    assert tot > 100


def test_local_lines_at_mlcap_32768():
    """256 keylines and 32768 local map lines, 16 levels, predicted levels up to 16 and the window ends -1 / nlevels / nlevels + 1,
    keyline octaves outside [0, 16).  k_line_assign<true>'s LDS holds short[mlcap] = 64 KiB next to the keyline tiles."""
    from manhattanslam_amd import match
    p = lsc.params(1.0, nlevels=16)
    c, l, T = lsc.local_frame(1401, p, n_kl=256, n_local=32768, octaves=16)
    c["kl"]["octave"][3::29] = np.resize([-1, 16, 99], len(c["kl"]["octave"][3::29]))
    c2, l2, T2 = lsc.local_frame(1402, p, n_kl=100, n_local=3000, few=4, octaves=16)
    cur, local, Ts = [c, c2], [l, l2], np.stack([T, T2])
    init = _init_io(2, 256, 14)
    match_, ntm, nm, inv, trk, lx, lh = match.search_local_lines_batch(p, cur, local, Ts, lcap=256, mlcap=32768, line_xyz=init[0],
                                                                       line_has=init[1])
    for f in range(2):
        wm, wntm, wnm, winv, wtrk = lmm.search_local_lines(p, cur[f], local[f], Ts[f])
        assert ntm[f] == wntm and nm[f] == wnm, (f, ntm[f], wntm, nm[f], wnm)
        assert np.array_equal(match_[f], wm), (f, np.flatnonzero(match_[f] != wm)[:10])
        assert np.array_equal(inv[f], winv) and trk[f].tobytes() == wtrk.tobytes(), f
        wx, wh = lmm.pose_layout(wm, local[f]["xyz"], 256, init[0][f], init[1][f], clear=False)
        assert lx[f].tobytes() == wx.tobytes() and np.array_equal(lh[f], wh), f
    assert ntm[0] > 10000 and nm[0] > 50


# ---- 4. pose and translation at the top end -------------------------------------------------------------------------------------------
def _top_frame(seed, c, translation=False, rcw_out=None):
    """8192 keypoints with references scattered over 32768 xyz rows (up to 32767), 256 lines all present, 64 planes with all three kinds,
    octaves 0-15, a few octaves -1 / 16 / 99 / 1000 / INT_MIN and references 32768 / INT_MAX / -5 / INT_MIN."""
    kw = dict(n_pts=8192, n_lines=256, n_planes=64, nlevels=16, xcap=32768, c=c, margin=None)
    if translation:
        fr, rcw, _, _ = ts.scene(seed, **kw)
    else:
        fr, _, _ = ps.scene(seed, **kw)
    fr["line_has"][:] = 1
    ok = np.flatnonzero(fr["pt_ref"] >= 0)
    fr["octave"][ok[5::301]] = np.resize(BAD_OCTAVES, len(ok[5::301]))
    fr["pt_ref"][ok[7::401]] = np.resize([32768, 2 ** 31 - 1, -5, -2 ** 31], len(ok[7::401]))
    assert 32767 in fr["pt_ref"]
    if translation:
        ts.check_margin(fr, c, rcw)
        rcw_out.append(rcw)
    else:
        ps.check_margin(fr, c)
    return fr


def test_pose_at_the_top_end():
    from manhattanslam_amd import pose
    c = ps.params(nlevels=16, inv_level_sigma2=ms.orb_tables(16, 1.2)[1])
    frames = [_top_frame(1501, c), ps.scene(1502, n_pts=3000, n_lines=40, n_planes=0, nlevels=16, c=c)[0]]
    got = pose.pose_optimization_batch(pose.pose_params(c), frames, caps=(8192, 32768, 256, 64))
    _check_pose(c, frames, got)
    assert got[0][0] > 7000


def test_translation_at_the_top_end():
    from manhattanslam_amd import pose
    c = ps.params(nlevels=16, inv_level_sigma2=ms.orb_tables(16, 1.2)[1])
    rcw = []
    frames = [_top_frame(1601, c, True, rcw)]
    fr, r, _, _ = ts.scene(1602, n_pts=3000, n_lines=40, n_planes=4, nlevels=16, c=c)
    frames.append(fr); rcw.append(r)
    rcw = np.stack(rcw)
    got = pose.translation_optimization_batch(pose.pose_params(c), frames, rcw, caps=(8192, 32768, 256, 64))
    _check_pose(c, frames, got, tm.translation_optimization, rcw, planes=("plane",))
    assert got[0][0] > 7000


# ---- 5. poisoned tails and tables ----------------------------------------------------------------------------------------------------
def _poison(a, counts, rng):
    """a [frames][cap ...] with every row at or past counts[f] replaced by plausible but wrong data: shifted copies of that frame's real rows
    (or of the next frame's when it has none), every third such row of a float array NaN."""
    a = a.copy()
    F, cap = a.shape[:2]
    for f in range(F):
        n = int(counts[f])
        if n >= cap:
            continue
        g = f if n else next((g for g in range(1, F + 1) if counts[(f + g) % F]), None)
        if g is None:
            continue
        src_f = f if n else (f + g) % F
        src = np.roll(a[src_f, :int(counts[src_f])], int(rng.integers(1, 7)), axis=0)
        a[f, n:] = np.resize(src, (cap - n,) + a.shape[2:]) if src.dtype.fields is None else np.resize(src, cap - n)
        if a.dtype.kind == "f":
            a[f, n::3] = np.nan
    return a


def _run_twice(call, arrays, counts_of, io_init, p, table, nlevels):
    """call(params, inputs, outputs) twice: clean, then with the tail of inputs[i] past its counts poisoned for every i in counts_of (counts:
    the index of the input that holds them, or an array) and params' table (a field path) NaN from nlevels on.  Every output array, whole,
    must be bit-identical; returns the clean outputs."""
    rng = np.random.default_rng(99)
    res = []
    for poisoned in (False, True):
        q = p.copy()
        ins = [a.copy() for a in arrays]
        if poisoned:
            t = q
            for k in table:
                t = t[k]
            t[0, nlevels:] = np.nan
            for i, cnt in counts_of.items():
                ins[i] = _poison(ins[i], ins[cnt] if isinstance(cnt, int) else cnt, rng)
        outs = [o.copy() for o in io_init]
        call(q, ins, outs)
        res.append(outs)
    for k, (a, b) in enumerate(zip(*res)):
        assert a.tobytes() == b.tobytes(), (k, np.flatnonzero(a.reshape(len(a), -1) != b.reshape(len(b), -1))[:10])
    return res[0]


def _call(name):
    from manhattanslam_amd._lib import MSL_MEM_HOST, call, ptr

    def run(p, ins, outs, head=()):
        call(name, None, 0, *head, ptr(p), *[ptr(a) for a in ins], MSL_MEM_HOST, *[ptr(o) for o in outs], MSL_MEM_HOST)
    return run


def test_poisoned_tails_and_tables_points(oracle):
    """Last-frame and local point matching, 12 of 16 levels: tails past n_cur / n_last / n_local hold shifted copies of real keypoints,
    cells, descriptors and points (NaN in some rows), scale_factors[12:] NaN.  match_out over the whole [frames][cap], nmatches,
    n_to_match, in_view and track are bit-identical to the clean call, which equals the oracle / the model."""
    from manhattanslam_amd import match, LOCAL_TRACK_DTYPE, MATCH_PARAMS_DTYPE
    p = ms.params(None, 15, True, dtype=MATCH_PARAMS_DTYPE, nlevels=12)
    pairs = [ms.random_pair(1700 + j, p, n_cur=n, n_last=m, tz=tz) for j, (n, m, tz) in enumerate(((900, 300, 0.0), (200, 1000, 0.3), (1000, 1000, -0.3)))]
    cur, last = [q[0] for q in pairs], [q[1] for q in pairs]
    Tc, Tl = np.stack([q[2] for q in pairs]), np.stack([q[3] for q in pairs])
    cap = 1024
    arrays = match._pack_cur(cur, cap) + [match.pad(last, "xyz", cap, np.float32, shape=(3,)), match.pad(last, "desc", cap, np.uint8, shape=(32,)),
                                          match.pad(last, "flags", cap, np.uint8), match.pad(last, "octave", cap, np.int32),
                                          match.pad(last, "angle", cap, np.float32), np.array([len(l["xyz"]) for l in last], np.int32),
                                          match._rows3x4(Tc, 3), match._rows3x4(Tl, 3)]
    B = 3
    run = _call("msl_match_by_projection")
    out = _run_twice(lambda q, ins, outs: run(q, ins, outs, (B, cap)), arrays, {0: 5, 1: 5, 2: 5, 3: 5, 4: 5, 6: 11, 7: 11, 8: 11, 9: 11, 10: 11},
                     [np.full((B, cap), -7, np.int32), np.zeros(B, np.int32)], p, ("scale_factors",), 12)
    assert _check_points(p, cur, last, Tc, Tl, out[0], out[1]) > 500

    lp = ls.params(3.0, nlevels=12)
    frames = [ls.random_frame(1710 + j, lp, n_cur=n, n_local=m, **kw) for j, (n, m, kw) in
              enumerate(((800, 3000, {}), (300, 500, dict(preheld=0.5)), (1000, 2000, dict(conflict=True))))]
    cur, local, T = [q[0] for q in frames], [q[1] for q in frames], np.stack([q[2] for q in frames])
    cap, mcap, arrays = match.pack_local_points(cur, local, T, 1024, 4096)
    run = _call("msl_match_local_points")
    io = [np.full((B, cap), -7, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32), np.full((B, mcap), 5, np.uint8),
          np.zeros((B, mcap), LOCAL_TRACK_DTYPE)]
    out = _run_twice(lambda q, ins, outs: run(q, ins, outs, (B, cap, mcap)), arrays,
                     {0: 5, 1: 5, 2: 5, 3: 5, 4: 5, 6: 5, 7: 12, 8: 12, 9: 12, 10: 12, 11: 12}, io, lp, ("scale_factors",), 12)
    got = ([out[0][f, :len(cur[f]["kps"])] for f in range(B)], out[1], out[2], [out[3][f, :len(local[f]["xyz"])] for f in range(B)],
           [out[4][f, :len(local[f]["xyz"])] for f in range(B)])
    assert _check_local(lp, cur, local, T, got) > 500


def test_poisoned_tails_and_tables_lines():
    """Both line searches, 12 of 16 levels: keyline, line, descriptor and flag tails poisoned, scale_factors[12:] NaN.  match_out, counts,
    in_view, track, line_xyz and line_has over every slot are bit-identical to the clean call; slots past n_cur_lines keep their input."""
    from manhattanslam_amd import match, LINE_TRACK_DTYPE
    p = lsc.params(15.0, nlevels=12)
    pairs = [lsc.frame_pair(1800 + j, p, n_kl=n, n_last=m, octaves=12, fwd=fwd) for j, (n, m, fwd) in enumerate(((60, 30, 0.0), (20, 90, 0.4), (100, 100, -0.4)))]
    cur, last = [q[0] for q in pairs], [q[1] for q in pairs]
    Tc, Tl = np.stack([q[2] for q in pairs]), np.stack([q[3] for q in pairs])
    lcap, llcap, arrays = match.pack_lines_last(cur, last, Tc, Tl, 128, 128)
    B = 3
    lx0, lh0 = _init_io(B, lcap, 18)
    run = _call("msl_match_lines_by_projection")
    out = _run_twice(lambda q, ins, outs: run(q, ins, outs, (B, lcap, llcap)), arrays, {0: 2, 1: 2, 3: 7, 4: 7, 5: 7, 6: 7},
                     [np.full((B, lcap), -7, np.int32), np.zeros(B, np.int32), lx0, lh0], p, ("scale_factors",), 12)
    for f in range(B):
        n = len(cur[f]["kl"])
        wm, wnm = lmm.search_lines_by_projection(p, cur[f], last[f], Tc[f], Tl[f])
        assert out[1][f] == wnm and np.array_equal(out[0][f, :n], wm), f
        assert out[2][f, n:].tobytes() == lx0[f, n:].tobytes() and np.array_equal(out[3][f, n:], lh0[f, n:]), f

    lp = lsc.params(1.0, nlevels=12)
    frames = [lsc.local_frame(1810 + j, lp, n_kl=n, n_local=m, octaves=12) for j, (n, m) in enumerate(((80, 2000), (30, 300), (120, 1000)))]
    cur, local, T = [q[0] for q in frames], [q[1] for q in frames], np.stack([q[2] for q in frames])
    lcap, mlcap, arrays = match.pack_local_lines(cur, local, T, 128, 2048)
    lx0, lh0 = _init_io(B, lcap, 19)
    run = _call("msl_match_local_lines")
    io = [np.full((B, lcap), -7, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32), np.full((B, mlcap), 5, np.uint8),
          np.zeros((B, mlcap), LINE_TRACK_DTYPE), lx0, lh0]
    out = _run_twice(lambda q, ins, outs: run(q, ins, outs, (B, lcap, mlcap)), arrays, {0: 2, 1: 2, 3: 2, 4: 9, 5: 9, 6: 9, 7: 9, 8: 9},
                     io, lp, ("scale_factors",), 12)
    for f in range(B):
        n, m = len(cur[f]["kl"]), len(local[f]["xyz"])
        wm, wntm, wnm, winv, wtrk = lmm.search_local_lines(lp, cur[f], local[f], T[f])
        assert out[1][f] == wntm and out[2][f] == wnm and np.array_equal(out[0][f, :n], wm), f
        assert np.array_equal(out[3][f, :m], winv) and out[4][f, :m].tobytes() == wtrk.tobytes(), f
        wx, wh = lmm.pose_layout(wm, local[f]["xyz"], lcap, lx0[f], lh0[f], clear=False)
        assert out[5][f].tobytes() == wx.tobytes() and np.array_equal(out[6][f], wh), f


@pytest.mark.parametrize("translation", [False, True])
def test_poisoned_tails_and_tables_pose(translation):
    """Pose (and translation) optimisation, 12 of 16 levels: keypoint, reference, point, line and plane tails poisoned (the references
    past n_kps point at real rows), inv_level_sigma2[12:] NaN.  Tcw_out, n_good and the three outlier arrays over every slot are
    bit-identical to the clean call, slots without an edge keep their input, and the clean call equals the model."""
    from manhattanslam_amd import pose
    c = ps.params(nlevels=12, inv_level_sigma2=ms.orb_tables(12, 1.2)[1])
    specs = [dict(seed=1901, n_pts=500, n_lines=10, n_planes=3), dict(seed=1902, n_pts=80, n_lines=0, n_planes=1),
             dict(seed=1903, n_pts=1200, n_lines=30, n_planes=0)]
    if translation:
        sc = [ts.scene(nlevels=12, c=c, **s) for s in specs]
        frames, rcw = [q[0] for q in sc], np.stack([q[1] for q in sc]).astype(np.float32)
    else:
        frames, rcw = [ps.scene(nlevels=12, c=c, **s)[0] for s in specs], None
    caps, arrays, io = pose.pack(frames, 1536, 1536, 64, 8)
    F = len(frames)
    name = "msl_pose_optimize_translation" if translation else "msl_pose_optimize"
    from manhattanslam_amd._lib import MSL_MEM_HOST, call, ptr

    def run(q, ins, outs):
        extra = [ptr(np.ascontiguousarray(rcw))] if translation else []
        call(name, None, 0, F, *caps, ptr(q), *[ptr(a) for a in ins], *extra, MSL_MEM_HOST, *[ptr(o) for o in outs], MSL_MEM_HOST)
    rng = np.random.default_rng(5)
    io = [rng.integers(0, 2, a.shape).astype(np.uint8) for a in io]
    p = pose.pose_params(c)
    out = _run_twice(run, arrays, {0: 4, 1: 4, 2: 4, 3: 4, 5: np.array([len(f["xyz"]) for f in frames]), 6: 9, 7: 9, 8: 9, 10: 13, 11: 13, 12: 13},
                     io + [np.zeros((F, 12), np.float32), np.zeros(F, np.int32)], p, ("inv_level_sigma2",), 12)
    for f, fr in enumerate(frames):
        n, nl, m = len(fr["pt_ref"]), len(fr["line_has"]), len(fr["plane_coef"])
        assert np.array_equal(out[0][f, n:], io[0][f, n:]) and np.array_equal(out[1][f, nl:], io[1][f, nl:])
        assert np.array_equal(out[2][f, m:], io[2][f, m:])
    got = pose.unpack(frames, out[:3], out[3], out[4])
    init = pose.unpack(frames, io, out[3], out[4])
    for f, fr in enumerate(frames):                                               # the model starts from the same flags
        for k, v in init[f][2].items():
            fr[k] = v
    if translation:
        _check_pose(c, frames, got, tm.translation_optimization, rcw, planes=("plane",))
    else:
        _check_pose(c, frames, got)


# ---- 6. wide batches ---------------------------------------------------------------------------------------------------------------------
def test_wide_pose_and_translation_batches():
    """264 small ragged frames in one call (more workgroups than the device has CUs), pose and translation form: every frame equals the
    model and its own 1-frame call."""
    from manhattanslam_amd import pose
    c = ps.params()
    p = pose.pose_params(c)
    rng = np.random.default_rng(2001)
    sc = [ts.scene(2100 + f, n_pts=int(rng.integers(0, 60)), n_lines=int(rng.integers(0, 5)), n_planes=int(rng.integers(0, 3)), c=c)
          for f in range(264)]
    frames, rcw = [q[0] for q in sc], np.stack([q[1] for q in sc])
    for form, model, kw in ((pose.pose_optimization_batch, pm.pose_optimization, {}),
                            (pose.translation_optimization_batch, tm.translation_optimization, dict(rcw=rcw))):
        got = form(p, frames, **kw)
        if kw:
            _check_pose(c, frames, got, model, rcw, planes=("plane",))
        else:
            for fr in frames:                                                     # ts.scene checked the translation model's margins
                ps.check_margin(fr, c)
            _check_pose(c, frames, got)
        for f in range(0, 264, 11):
            one = form(p, [frames[f]], **({"rcw": rcw[f:f + 1]} if kw else {}))[0]
            assert one[0] == got[f][0] and one[1].tobytes() == got[f][1].tobytes(), f
            assert all(np.array_equal(one[2][k], got[f][2][k]) for k in one[2]), f


def test_wide_point_search_batches(oracle):
    """300 ragged pairs for the last-frame search and 300 frames for the local search in one call each: every frame equals the oracle / the
    model and its own 1-frame call."""
    from manhattanslam_amd import match, MATCH_PARAMS_DTYPE
    rng = np.random.default_rng(2002)
    p = ms.params(None, 15, True, dtype=MATCH_PARAMS_DTYPE)
    pairs = [ms.random_pair(2200 + f, p, n_cur=int(rng.integers(1, 200)), n_last=int(rng.integers(1, 200)), tz=float(rng.choice([0.0, 0.3, -0.3])))
             for f in range(300)]
    cur, last = [q[0] for q in pairs], [q[1] for q in pairs]
    Tc, Tl = np.stack([q[2] for q in pairs]), np.stack([q[3] for q in pairs])
    got, nm = match.search_by_projection_batch(p, cur, last, Tc, Tl)
    assert _check_points(p, cur, last, Tc, Tl, got, nm) > 3000
    for f in range(0, 300, 13):
        one, n1 = match.search_by_projection_batch(p, cur[f:f + 1], last[f:f + 1], Tc[f:f + 1], Tl[f:f + 1])
        assert n1[0] == nm[f] and np.array_equal(one[0], got[f]), f

    lp = ls.params()
    frames = [ls.random_frame(2300 + f, lp, n_cur=int(rng.integers(0, 150)), n_local=int(rng.integers(1, 400))) for f in range(300)]
    cur, local, T = [q[0] for q in frames], [q[1] for q in frames], np.stack([q[2] for q in frames])
    got = match.search_local_points_batch(lp, cur, local, T)
    assert _check_local(lp, cur, local, T, got) > 3000
    for f in range(0, 300, 13):
        one = match.search_local_points_batch(lp, cur[f:f + 1], local[f:f + 1], T[f:f + 1])
        assert one[1][0] == got[1][f] and one[2][0] == got[2][f] and np.array_equal(one[0][0], got[0][f]), f
        assert np.array_equal(one[3][0], got[3][f]) and one[4][0].tobytes() == got[4][f].tobytes(), f


# ---- 7. the largest pyramid the extractor makes ----------------------------------------------------------------------------------------
def test_matching_consumes_12_level_orb_frames(oracle):
    """ORBextractor with 12 levels of 1.1 (the extractor's level limit): its device frame outputs and msl_orb_scale_tables feed
    msl_match_by_projection, which equals the oracle; the keypoints span all 12 octaves."""
    from manhattanslam_amd import ORBextractor, frame_params, match, synth
    from tests import oracle_lib
    I = synth.TUM1
    img0 = synth.orb_frame(synth.ORB_SEED + 23)
    img1 = np.roll(img0, (2, 4), axis=(0, 1))
    depth = np.full((480, 640), 2.0, np.float32)
    fp = frame_params(I["fx"], I["fy"], I["cx"], I["cy"], 40.0, 640, 480)
    ex = ORBextractor(2000, 1.1, 12, 20, 7, max_batch=2)
    (k0, d0, un0, z0, ur0, c0), (k1, d1, un1, z1, ur1, c1) = ex.extract_frames(np.stack([img0, img1]), np.stack([depth, depth]), fp)
    sf = ex.GetScaleFactors()
    ex.close()
    assert len(sf) == 12 and np.array_equal(np.asarray(sf, np.float32), ms.orb_tables(12, 1.1)[0])
    assert set(np.unique(k1["octave"])) == set(range(12))
    xyz = np.stack([(un0[:, 0] - I["cx"]) * z0 / I["fx"], (un0[:, 1] - I["cy"]) * z0 / I["fy"], z0], 1).astype(np.float32)
    rng = np.random.default_rng(4)
    last = dict(xyz=xyz, desc=d0, flags=((z0 > 0).astype(np.uint8) | ((rng.random(len(k0)) < 0.6).astype(np.uint8) << 1)), octave=k0["octave"],
                angle=k0["angle"])
    cur = dict(kps=k1, un_xy=un1, uright=ur1, grid_cell=c1, desc=d1)
    Tl = np.eye(4, dtype=np.float32)
    for tz in (0.0, 0.2, -0.2):
        Tc = np.eye(4, dtype=np.float32)
        Tc[0, 3] = 4 * 2.0 / I["fx"]; Tc[1, 3] = 2 * 2.0 / I["fy"]; Tc[2, 3] = tz
        p = match.match_params(fp, sf, 15.0, True)
        got, nm = match.search_by_projection_batch(p, [cur], [last], Tc[None], Tl[None])
        want, n = oracle_lib.search_by_projection(p, cur, last, Tc, Tl)
        assert nm[0] == n and np.array_equal(got[0], want), tz
        if tz == 0.0:
            assert n > 500

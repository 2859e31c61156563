"""msl_fuse_map_lines on the device against its sequential model (tests/linefuse_model.py) on the keyframe graphs of
tests/linefuse_scenes.py: every output exactly, the debug accessor's u1, v1, u2, v2 and radius as bytes (the kernels run the model's
operations in the model's order, contraction off; tests/test_linefuse_model.py::test_margins keeps every comparison away from its
threshold all the same)."""
import numpy as np
import pytest

from tests import linefuse_model as lf
from tests import linefuse_scenes as ls

pytestmark = pytest.mark.gpu
MSL_ERR_INVALID = -1
F32 = np.float32


def _params(p):
    from manhattanslam_amd import linefuse
    return linefuse.line_fuse_params(p["fx"], p["fy"], p["cx"], p["cy"], p["minX"], p["maxX"], p["minY"], p["maxY"], p["scale_factors"],
                                     p["log_scale_factor"], th=p["th"], th_low=p["th_low"])


@pytest.fixture(scope="module")
def matcher():
    from manhattanslam_amd.match import Matcher
    h = Matcher()
    yield h
    h.close()


def _check(got, f, res, n):
    """Item f of the device's outputs against the model's result for a list of n candidates."""
    for k in ("best_idx", "best_dist", "status", "other"):
        bad = got[k][f, :n] != res[k]
        assert not bad.any(), (f, k, np.flatnonzero(bad)[:8], got[k][f, :n][bad][:8], np.asarray(res[k])[bad][:8])
    assert int(got["n_fused"][f]) == res["n_fused"], (f, got["n_fused"][f], res["n_fused"])
    # slots beyond the count: -1 for indices, 0 for everything else
    assert (got["best_idx"][f, n:] == -1).all() and (got["other"][f, n:] == -1).all() and not got["best_dist"][f, n:].any() and not got["status"][f, n:].any()
    return res["n_fused"]


def _check_debug(handle, f, res, lcap):
    from manhattanslam_amd import linefuse
    d = linefuse.debug_line_fuse(handle, f, lcap)
    n = len(res["trace"])
    for k, dt in (("u1", F32), ("v1", F32), ("u2", F32), ("v2", F32), ("radius", F32), ("level", np.int32), ("n_indices", np.int32)):
        want = np.array([tr[k] for tr in res["trace"]], dt)
        assert d[k][:n].tobytes() == want.tobytes(), (f, k, np.flatnonzero(d[k][:n].view(np.int32) != want.view(np.int32))[:8])
        assert not d[k][n:].any()


def _ragged():
    """The state of graph a on entry with keyframes of 0, 1, 63, 64 and 65 keylines cut from the one of 256 (the others have at most 40),
    and the line table doubled by shifted copies so that lists of 0, 1, 63, 64, 65 and lcap candidates exist; one list of NULLs only, and
    the current keyframe's own list shared by five targets."""
    table, lines, _ = ls.runs("a")["entry"]
    n = len(lines["flags"])
    r = np.random.RandomState(5)
    shifted = lines["xyz"] + np.tile(r.normal(0, 0.004, (n, 3)), 2)
    lines = {k: np.concatenate([v, shifted if k == "xyz" else v]) for k, v in lines.items()}
    big = table[ls.BIG]
    cut = lambda m: {k: (v if k == "Tcw" else v[:m]) for k, v in big.items()}
    base = len(table)
    table = list(table) + [cut(0), cut(1), cut(63), cut(64), cut(65)]
    full = [int(i) for i in r.permutation(2 * n)]
    own = [int(h) for h in table[ls.CUR]["held_id"]]
    seen = set()
    own = [(-1 if (p in seen or seen.add(p)) else p) if p >= 0 else -1 for p in own]
    lists = [[], full[:1], full[:63], full[:64], full[:65], full, [-1] * 10, own]
    items = [(ls.CUR, l) for l in range(7)] + [(t, 7) for t in (1, 2, 3, 4, 5)] + [(base + i, 5) for i in range(5)] + [(ls.BIG, 5), (7, 5)]
    return table, lines, items, lists


def test_ragged_batch_matches_model(matcher):
    from manhattanslam_amd import linefuse
    table, lines, items, lists = _ragged()
    lcap = max(len(l) for l in lists)
    assert {0, 1, 10, 63, 64, 65, lcap} <= {len(l) for l in lists} and lcap > 65
    assert {0, 1, 63, 64, 65, 256} <= {len(k["kl"]) for k in table} and len(table[ls.CUR]["kl"]) <= 40
    got = linefuse.fuse_map_lines(_params(ls.prm()), table, lines, items, lists, handle=matcher)
    assert got["status"].shape == (len(items), lcap)
    res = lf.fuse_map_lines(ls.prm(), table, lines, items, lists)
    fused = sum(_check(got, f, res[f], len(lists[l])) for f, (_, l) in enumerate(items))
    assert fused > 60
    assert (got["status"][6, :10] == lf.NULL).all() and (got["best_dist"][6, :10] == lf.INT_MAX).all() and got["n_fused"][6] == 0
    assert not got["n_fused"][12]                                            # no keylines: nothing fused
    assert (got["status"][12, :lcap] <= lf.NO_FEATURE).all()
    for f, (_, l) in enumerate(items):
        _check_debug(matcher, f, res[f], lcap)


@pytest.mark.parametrize("name", ls.ALL)
def test_coverage_scenes_match_model(matcher, name):
    """Both Fuse calls of SearchInNeighbors on every graph, the first with its seven targets sharing one list."""
    from manhattanslam_amd import linefuse
    seen, n = set(), 0
    for table, lines, items, lists, res in ls.runs(name)["calls"]:
        if len(lists[0]) == 1:
            continue                                                           # the single-candidate searches of the replay
        got = linefuse.fuse_map_lines(_params(ls.prm()), table, lines, items, lists, handle=matcher)
        for f, (_, l) in enumerate(items):
            _check(got, f, res[f], len(lists[l]))
            _check_debug(matcher, f, res[f], got["status"].shape[1])
            seen |= set(got["status"][f, :len(lists[l])].tolist())
        n += 1
    assert n == 2 and seen == set(range(15))


def _edge_case():
    """One identity-pose keyframe with keylines far apart and hand-placed lines; returns (prm, table, lines, list)."""
    from manhattanslam_amd import KEYLINE_DTYPE
    p = ls.prm()
    z = 4.0
    X = lambda u: (u - ls.CX) / ls.FX * z
    Y = lambda v: (v - ls.CY) / ls.FY * z
    kl_rows, xyz, dist, desc = [], [], [], []

    def keyline(u, v, angle, octave, byte):
        kl_rows.append((u, v, angle, octave, byte))

    def line(P, dmin=None, dmax=None, d=None):
        P = np.asarray(P, np.float64)
        mid = 0.5 * (P[:3] + P[3:])
        n = float(np.linalg.norm(mid))
        xyz.append(P); dist.append((n * 0.9 / 1.2 ** 7 if dmin is None else dmin, n * 0.9 if dmax is None else dmax))
        desc.append(np.zeros(32, np.uint8) if d is None else d)

    def bits(n):
        d = np.zeros(32, np.uint8)
        d[:n // 8] = 0xFF
        if n % 8:
            d[n // 8] = (1 << (n % 8)) - 1
        return d
    keyline(40.0, 40.0, 5.0, 0, 0)                                               # 0: angle 5 passes every finite slope
    line([X(30.0), Y(40.0), z, X(50.0), Y(40.0), z])                              # 0: a plain hit on keyline 0 (ADDED)
    line([0.0, 0.0, 0.0, X(50.0), Y(40.0), z])                                    # 1: SP at the camera centre: Z == 0, 0 * inf = NaN passes the bounds
    line([0.5, 0.5, 0.0, X(50.0), Y(40.0), z])                                    # 2: Z == 0 off the axis: +inf, outside
    keyline(100.0, 60.0, 5.0, 0, 0)                                              # 1
    line([X(100.0), Y(50.0), z, X(100.0), Y(70.0), z])                            # 3: u1 == u2, v1 < v2: slope -inf passes
    line([X(100.0), Y(70.0), z, X(100.0), Y(50.0), z])                            # 4: u1 == u2, v1 > v2: slope +inf fails
    line([X(100.0), Y(60.0), z, X(100.0), Y(60.0), z])                            # 5: a point: 0 / 0 = NaN passes
    keyline(200.0, 60.0, 5.0, 0, 0)                                              # 2: octave 0
    keyline(200.0, 61.0, 5.0, 10, 0)                                             # 3: octave 10, outside the pyramid
    n200 = float(np.linalg.norm([X(200.0), Y(60.0), z]))
    line([X(190.0), Y(60.0), z, X(210.0), Y(60.0), z], dmin=0.0, dmax=float("nan"))                 # 6: NaN range: level INT_MIN, the window wraps
    line([X(190.0), Y(60.0), z, X(210.0), Y(60.0), z], dmin=0.0, dmax=n200 * 1.2 ** 9.5)            # 7: level 10 >= nlevels: radius of level 7, octave 10 only
    line([X(190.0), Y(60.0), z, X(210.0), Y(60.0), z], dmin=0.0, dmax=n200 * 1.2 ** 12.5)           # 8: level 13: nothing in the window
    keyline(260.0, 180.0, 5.0, 0, 0)                                             # 4
    line([X(250.0), Y(180.0), z, X(270.0), Y(180.0), z], d=bits(50))              # 9: exactly th_low
    line([X(250.0), Y(180.0), z, X(270.0), Y(180.0), z], d=bits(51))              # 10: th_low + 1
    line([X(250.0), Y(180.0), z, X(270.0), Y(180.0), z], d=bits(256))             # 11: distance 256 is a distance, not "none"
    kl = np.zeros(len(kl_rows), KEYLINE_DTYPE)
    kl["x"] = [k[0] for k in kl_rows]; kl["y"] = [k[1] for k in kl_rows]; kl["angle"] = [k[2] for k in kl_rows]; kl["octave"] = [k[3] for k in kl_rows]
    table = [dict(kl=kl, ldesc=np.zeros((len(kl), 32), np.uint8), Tcw=np.eye(4, dtype=F32)[:3], held_id=np.full(len(kl), -1, np.int32))]
    m = len(xyz)
    mids = [0.5 * (P[:3] + P[3:]) for P in xyz]
    lines = dict(xyz=np.array(xyz), normal=np.array([c / np.linalg.norm(c) for c in mids]), dist=np.array(dist, F32), desc=np.array(desc, np.uint8),
                 flags=np.ones(m, np.uint8), nobs=np.arange(1, m + 1, dtype=np.int32))
    return p, table, lines, list(range(m))


def test_edge_arithmetic(matcher):
    """Non-finite projections and slopes, levels outside the pyramid, the th_low boundary and distance 256: the model decides, the device
    agrees."""
    from manhattanslam_amd import linefuse
    p, table, lines, lst = _edge_case()
    res = lf.fuse_item(p, table[0], lines, lst)
    st, bd, bi, tr = res["status"].tolist(), res["best_dist"].tolist(), res["best_idx"].tolist(), res["trace"]
    # what the model decides (the reference's arithmetic, written down once)
    assert st[0] == lf.ADDED and bi[0] == 0
    assert np.isnan(tr[1]["u1"]) and np.isnan(tr[1]["v1"]) and tr[1]["n_indices"] == len(table[0]["kl"]) and st[1] >= lf.ADDED   # NaN midpoint: every keyline
    assert st[2] == lf.OUT_OF_IMAGE
    assert tr[3]["u1"] == tr[3]["u2"] and tr[3]["n_indices"] == 1 and bi[3] == 1
    assert tr[4]["u1"] == tr[4]["u2"] and st[4] == lf.NO_FEATURE
    assert tr[5]["v1"] == tr[5]["v2"] and tr[5]["n_indices"] == 1 and bi[5] == 1
    assert tr[6]["level"] == -2 ** 31 and tr[6]["radius"] == p["th"] * p["scale_factors"][0] and st[6] == lf.NO_CANDIDATE and bd[6] == lf.INT_MAX
    assert tr[7]["level"] == 10 and tr[7]["radius"] == p["th"] * p["scale_factors"][7] and tr[7]["n_indices"] == 2 and bi[7] == 3
    assert tr[8]["level"] == 13 and st[8] == lf.NO_CANDIDATE
    assert (bd[9], bd[10], bd[11]) == (50, 51, 256) and st[9] >= lf.ADDED and st[10] == lf.ABOVE_TH_LOW and st[11] == lf.ABOVE_TH_LOW and bi[11] == 4
    got = linefuse.fuse_map_lines(_params(p), table, lines, [(0, 0)], [lst], handle=matcher)
    _check(got, 0, res, len(lst))
    _check_debug(matcher, 0, res, len(lst))
    # th_low = 256, the largest the ABI accepts: distance 256 is accepted
    q = dict(p, th_low=256)
    res = lf.fuse_item(q, table[0], lines, lst)
    assert res["status"][11] >= lf.ADDED
    got = linefuse.fuse_map_lines(_params(q), table, lines, [(0, 0)], [lst], handle=matcher)
    _check(got, 0, res, len(lst))


class DeviceEntry(lf.ModelEntry):
    """The batched entries of the replay on the device (host memory)."""

    def __init__(self, handle):
        lf.ModelEntry.__init__(self)
        self.h = handle

    def candidates(self, table, lines, items):
        """msl_fuse_candidates over the line held_id and ln_flags with cap = klcap."""
        from manhattanslam_amd import linefuse
        from manhattanslam_amd._lib import lib, check, ptr
        klcap, t = linefuse.pack_line_table(table)
        n_lines, p = linefuse.pack_lines(lines)
        tcap = max(len(i) for i in items)
        targets = np.full((len(items), tcap), -1, np.int32)
        for f, it in enumerate(items):
            targets[f, :len(it)] = it
        n_targets = np.array([len(i) for i in items], np.int32)
        lcap = tcap * klcap
        cand = np.zeros((len(items), lcap), np.int32); n_cand = np.zeros(len(items), np.int32)
        check(lib.msl_fuse_candidates(self.h.h, len(table), klcap, n_lines, len(items), tcap, lcap, ptr(t["held_id"]), ptr(t["n_kl"]), ptr(p["ln_flags"]),
                                      ptr(targets), ptr(n_targets), 0, ptr(cand), ptr(n_cand), 0), "msl_fuse_candidates")
        return [cand[f, :n_cand[f]].tolist() for f in range(len(items))]

    def fuse(self, prm, table, lines, items, lists):
        from manhattanslam_amd import linefuse
        got = linefuse.fuse_map_lines(_params(prm), table, lines, items, lists, handle=self.h)
        return [dict({k: got[k][f, :len(lists[l])] for k in ("best_idx", "best_dist", "status", "other")}, n_fused=int(got["n_fused"][f]))
                for f, (_, l) in enumerate(items)]

    def refresh(self, g, prm, ids):
        """msl_refresh_map_points(MSL_REFRESH_DESC) over the line descriptors, then msl_refresh_map_lines, written into the objects."""
        from manhattanslam_amd import linefuse, mappoint
        if not ids:
            return
        table, lines = g.table(), g.lines()
        obs = [ml.observations() for ml in g.mls]
        rp = mappoint.refresh_params(prm["scale_factors"])
        d = mappoint.refresh_map_points(rp, [dict(desc=k["ldesc"]) for k in table], obs, dict(flags=lines["flags"]), ids, what=mappoint.REFRESH_DESC,
                                        handle=self.h)
        n = linefuse.refresh_map_lines(rp, table, obs, lines, ids, handle=self.h)
        for f, i in enumerate(ids):
            ml = g.mls[i]
            if d["status"][f] & mappoint.DESC_WRITTEN:
                ml.desc = d["out_desc"][f].copy()
            if n["status"][f] == lf.NORMAL_WRITTEN:
                ml.normal, ml.dist = n["out_normal"][f].copy(), n["out_dist"][f].copy()


@pytest.mark.parametrize("name", ls.ALL)
def test_replay_with_device_results(matcher, name):
    """Device search, candidate list and refresh, then linefuse_model.replay: the graph and the return values of the literal function.
    Survivors searched again go through a one-item device call."""
    g, p, cur, targets = ls.graph(name)
    entry = DeviceEntry(matcher)
    rets, stats = lf.replay(g, p, cur, targets, entry)
    lit_rets, lit_snap = ls.runs(name)["literal"]
    snap = g.snapshot()
    assert rets == lit_rets and snap["slots"] == lit_snap["slots"] and snap["lines"] == lit_snap["lines"]
    assert stats == ls.runs(name)["replay"][1]
    assert stats["researched"] >= 1


def test_limits_refused(matcher):
    """Every limit of msl.h at its value (accepted, tiny shapes otherwise) and one above it (MSL_ERR_INVALID, outputs untouched); an index
    outside its table and a list that holds a line twice are refused in host memory."""
    from manhattanslam_amd import linefuse
    from manhattanslam_amd._lib import KEYLINE_DTYPE, lib, ptr
    p, table, lines, lst = _edge_case()
    prm = _params(p)
    fill = lambda shape, dt: np.full(int(np.prod(shape)) * np.dtype(dt).itemsize, 0x5A, np.uint8).view(dt).reshape(shape)

    def call(klcap=8, n_tab=1, n_lines=None, n_items=1, lcap=None, prm=prm, items=((0, 0),), lists=(lst,)):
        n_lines = n_lines or len(lst)
        t = dict(kl=np.zeros((n_tab, klcap), KEYLINE_DTYPE), ldesc=np.zeros((n_tab, klcap, 32), np.uint8), n_kl=np.zeros(n_tab, np.int32),
                 Tcw=np.tile(np.eye(4, dtype=F32)[:3].reshape(12), (n_tab, 1)), held_id=np.full((n_tab, klcap), -1, np.int32))
        m = min(klcap, len(table[0]["kl"]))
        t["kl"][0, :m] = table[0]["kl"][:m]; t["n_kl"][0] = m
        _, ln = linefuse.pack_lines(lines)
        if n_lines > len(lst):
            ln = {k: np.concatenate([v, np.zeros((n_lines - len(lst),) + v.shape[1:], v.dtype)]) for k, v in ln.items()}
        lc, cand, n_cand = linefuse.pack_lists([list(l) for l in lists], lcap if lcap and lcap <= 65536 else None)
        tgt = np.zeros(n_items, np.int32); li = np.zeros(n_items, np.int32)
        tgt[:len(items)] = [i[0] for i in items]; li[:len(items)] = [i[1] for i in items]
        out = linefuse.outputs(min(n_items, 4096), lc, zeros=fill)
        rc = lib.msl_fuse_map_lines(matcher.h, n_tab, klcap, n_lines, n_items, len(cand), lcap or lc, ptr(prm), *[ptr(t[k]) for k in linefuse.TABLE_KEYS],
                                    *[ptr(ln[k]) for k in linefuse.LINE_KEYS], ptr(tgt), ptr(li), ptr(cand), ptr(n_cand), 0,
                                    *[ptr(out[k]) for k in linefuse.OUT_KEYS], 0)
        return rc, all((v.view(np.uint8) == 0x5A).all() for v in out.values())

    assert call() == (0, False)
    for kw in (dict(klcap=256), dict(n_tab=4096), dict(n_lines=1048576), dict(n_items=4096), dict(lcap=65536)):
        assert call(**kw) == (0, False), kw
    for kw, word in ((dict(klcap=257), b"klcap"), (dict(n_tab=4097), b"n_tab"), (dict(n_lines=1048577), b"n_lines"), (dict(n_items=4097), b"n_items"),
                     (dict(lcap=65537), b"lcap")):
        assert call(**kw) == (MSL_ERR_INVALID, True) and word in lib.msl_last_error(), kw
    for k, v, ok in (("nlevels", 16, True), ("nlevels", 17, False), ("nlevels", 0, False), ("th_low", 256, True), ("th_low", 0, True), ("th_low", 257, False),
                     ("th_low", -1, False)):
        q = prm.copy(); q[k] = v
        if k == "nlevels" and ok:
            q["scale_factors"][0, 8:] = q["scale_factors"][0, 7]
        assert call(prm=q) == ((0, False) if ok else (MSL_ERR_INVALID, True)), (k, v)
        assert ok or k.encode() in lib.msl_last_error()
    assert call(lists=[lst + [lst[0]]]) == (MSL_ERR_INVALID, True) and b"twice" in lib.msl_last_error()
    assert call(lists=[lst + [-1, -1]])[0] == 0                               # NULLs may repeat
    assert call(lists=[lst + [len(lst)]]) == (MSL_ERR_INVALID, True)
    assert call(lists=[lst + [-2]]) == (MSL_ERR_INVALID, True)
    assert call(items=[(1, 0)]) == (MSL_ERR_INVALID, True)
    assert call(items=[(-1, 0)]) == (MSL_ERR_INVALID, True)
    assert call(items=[(0, 1)]) == (MSL_ERR_INVALID, True)


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype.names:
        a = a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,))
    return torch.from_numpy(a).cuda()


def test_batch_form_equals_handle_form(matcher):
    """Host memory on the handle, the _batch form, and device memory on a caller's stream: the same bytes."""
    import torch
    from manhattanslam_amd import linefuse
    from manhattanslam_amd.match import Matcher
    table, lines, items, lists, _ = ls.runs("b")["calls"][0]
    prm = _params(ls.prm())
    klcap, lcap = 256, len(lists[0]) + 5
    host = linefuse.fuse_map_lines(prm, table, lines, items, lists, handle=matcher, klcap=klcap, lcap=lcap)
    batch = linefuse.fuse_map_lines(prm, table, lines, items, lists, klcap=klcap, lcap=lcap)
    h2 = Matcher()
    s = torch.cuda.Stream()
    h2.set_stream(s.cuda_stream)
    _, t = linefuse.pack_line_table(table, klcap)
    n_lines, p = linefuse.pack_lines(lines)
    _, cand, n_cand = linefuse.pack_lists(lists, lcap)
    with torch.cuda.stream(s):
        ins = [_dev(np.array([i[0] for i in items], np.int32)), _dev(np.array([i[1] for i in items], np.int32)), _dev(cand), _dev(n_cand)]
        d_t = {k: _dev(v) for k, v in t.items()}; d_p = {k: _dev(v) for k, v in p.items()}
        out = linefuse.outputs(len(items), lcap, zeros=lambda shape, dt: torch.full(shape, 0x5A, dtype=getattr(torch, np.dtype(dt).name), device="cuda"))
        linefuse.fuse_map_lines_device(h2, prm, len(table), klcap, n_lines, len(items), len(cand), lcap, d_t, d_p, *ins, out)
        total = out["n_fused"].sum()                                          # ordered behind the call by the stream alone
    s.synchronize()
    for k in linefuse.OUT_KEYS:
        assert batch[k].tobytes() == host[k].tobytes(), k
        assert out[k].cpu().numpy().tobytes() == host[k].tobytes(), k
    assert int(total) == int(host["n_fused"].sum()) > 20
    h2.close()


def test_device_chain_lines(matcher):
    """One handle, one stream, device tensors throughout: msl_lines_3d on frame t gives the line table rows (id = keyline index of the new
    keyframe 0); msl_refresh_map_lines gives them normal and distances; msl_fuse_candidates over keyframe 0 and msl_fuse_map_lines fuse
    them into keyframes 1 and 2.  The replay is host bookkeeping (the observation maps live with the caller); its observation table and
    flags go back up, msl_refresh_map_points(MSL_REFRESH_DESC) and msl_refresh_map_lines refresh the device line table in place, and
    msl_match_local_lines reads that table for frame t + 1.  The matches equal those of the literal models run end to end on the host."""
    import torch
    from manhattanslam_amd import KEYLINE_DTYPE, line3d, linefuse, mappoint
    from manhattanslam_amd import fuse as pfuse
    from manhattanslam_amd.match import Matcher, pack_local_lines
    from tests import line3d_model as l3
    from tests import line_match_model as lmm
    from tests import line_match_scenes as lsc
    from tests.test_line3d_gpu import KEYS, _chain_frames
    lcap = 32
    pll, prm3, t_frames, models, cur, last, Tc, Tl = _chain_frames(1, 20, lcap)
    m, base, octave, ends0, T0 = models[0], last[0]["desc"], last[0]["octave"], t_frames[0]["line_ends"], Tl[0]
    nk = len(octave)
    q = lmm._p(pll)
    p = lf.params(q["fx"], q["fy"], q["cx"], q["cy"], q["minX"], q["maxX"], q["minY"], q["maxY"])
    assert p["scale_factors"].tobytes() == np.asarray(q["scale_factors"][:8], F32).tobytes() and p["log_scale_factor"] == q["log_scale_factor"]
    # the keyframe table: 0 = frame t itself, 1 and 2 a few centimetres on, their keylines next to the projections of the model's lines
    rng = np.random.Generator(np.random.PCG64(41))
    slope0 = (ends0[:, 1] - ends0[:, 3]) / (ends0[:, 0] - ends0[:, 2])
    table = [dict(kl=lsc.keylines(ends0[:, :2], ends0[:, 2:], octave, (slope0 + 0.1).astype(F32)), ldesc=base.copy(), Tcw=T0[:3, :4].copy())]
    for k, dt in ((1, [0.02, 0.01, -0.03]), (2, [-0.03, 0.02, 0.02])):
        T = T0.copy(); T[:3, 3] += np.array(dt, F32)
        xy1 = rng.uniform(20, 620, (nk, 2)); xy2 = rng.uniform(20, 460, (nk, 2))
        desc = rng.integers(0, 256, (nk, 32), dtype=np.uint8); slope = np.zeros(nk)
        for i in range(nk):
            uv = lsc._project(pll, T, m["line_xyz"][i]) if m["line_ok"][i] else None
            if uv is None or not np.all(np.isfinite(uv)) or uv[0] == uv[2] or i == 2 + k:   # one line of each keyframe finds no keyline
                continue
            xy1[i] = uv[:2] + rng.normal(0, 0.3, 2); xy2[i] = uv[2:] + rng.normal(0, 0.3, 2)
            desc[i] = lsc.desc_flip(rng, base[i], int(rng.integers(0, 20))) if i != 6 + k else desc[i]   # and one a foreign descriptor
            slope[i] = (uv[1] - uv[3]) / (uv[0] - uv[2])
        table.append(dict(kl=lsc.keylines(xy1, xy2, octave, (slope + rng.uniform(0.02, 0.2, nk)).astype(F32)), ldesc=desc, Tcw=T[:3, :4].copy()))
    fp = _params(p)
    rp = mappoint.refresh_params(p["scale_factors"])
    _, W, H, a = line3d.pack_lines(t_frames, lcap)
    klcap, t = linefuse.pack_line_table(table, lcap)
    desc0 = np.zeros((lcap, 32), np.uint8); desc0[:nk] = base
    cur0 = dict(cur[0], flags=np.zeros(nk, np.uint8))
    _, _, larr = pack_local_lines([cur0], [dict(xyz=np.zeros((lcap, 6)), normal=np.zeros((lcap, 3)), dist=np.zeros((lcap, 2), F32),
                                                desc=np.zeros((lcap, 32), np.uint8), flags=np.zeros(lcap, np.uint8))], Tc[:1], lcap=lcap, mlcap=lcap)
    h = Matcher()
    s = torch.cuda.Stream()
    h.set_stream(s.cuda_stream)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    tz = lambda shape, dt: z(shape, getattr(torch, np.dtype(dt).name))
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v.view(np.uint8) if v.dtype == KEYLINE_DTYPE else (v.view(np.int32) if v.dtype == np.uint32 else v))).cuda()
    host = lambda x: x.cpu().numpy()
    with torch.cuda.stream(s):
        d = {k: dev(v) for k, v in a.items()}
        d_t = {k: dev(v) for k, v in t.items()}
        o3 = dict(line_depth=z((1, lcap, 2), torch.float32), line_xyz=z((1, lcap, 6), torch.float64), line_ok=z((1, lcap), torch.uint8),
                  line_new=z((1, lcap), torch.uint8), n_support=z((1, lcap), torch.int32), n_new=z(1, torch.int32))
        ar = torch.arange(lcap + 1, dtype=torch.int32, device="cuda")
        obs1 = dict(obs_off=ar, obs_kf=z(lcap, torch.int32), obs_idx=ar[:lcap].contiguous())      # every row: seen by keyframe 0 at its own index
        ln = dict(ln_xyz=o3["line_xyz"][0], ln_normal=z((lcap, 3), torch.float64), ln_dist=z((lcap, 2), torch.float32), ln_desc=dev(desc0),
                  ln_flags=o3["line_ok"][0], ln_ref=z(lcap, torch.int32))
        r1 = linefuse.refresh_outputs(lcap, zeros=tz)
        targets, n_targets = z((1, 1), torch.int32), torch.ones(1, dtype=torch.int32, device="cuda")
        cand, n_cand = z((1, lcap), torch.int32), z(1, torch.int32)
        fout = linefuse.outputs(2, lcap, zeros=tz)
        tgt, lst = dev(np.array([1, 2], np.int32)), z(2, torch.int32)
        s.synchronize()                                                    # the uploads and fills are done
        line3d.lines_3d_device(h, line3d.line3d_params(**prm3), 1, lcap, l3.DEPTH_ORDER, d["line_ends"], d["n_lines"], d["depth"], 4 * W, 4 * W * H, W, H,
                               d["line_flags"], d["Tcw"], d["seed"], *[o3[k] for k in KEYS])
        linefuse.refresh_map_lines_device(h, rp, 3, klcap, lcap, lcap, lcap, d_t, obs1, ln, ar[:lcap].contiguous(), r1, ln)
        ok = o3["line_ok"][0] != 0
        ln["ln_nobs"] = ok.to(torch.int32)
        d_t["held_id"][0] = torch.where(ok, ar[:lcap], torch.full_like(ar[:lcap], -1))
        pfuse.fuse_candidates_device(h, 3, klcap, lcap, 1, 1, lcap, d_t["held_id"], d_t["n_kl"], ln["ln_flags"], targets, n_targets, cand, n_cand)
        linefuse.fuse_map_lines_device(h, fp, 3, klcap, lcap, 2, 1, lcap, d_t, ln, tgt, lst, cand, n_cand, fout)
        h.sync()
    # stage 1 against its model; then the host objects of the replay from the device's own table
    for k in ("line_xyz", "line_ok"):
        assert host(o3[k])[0, :nk].tobytes() == m[k].tobytes(), k
    okh = host(o3["line_ok"])[0].astype(bool)

    def graph(xyz, normal, dist):
        g = lf.Graph([dict(k) for k in table])
        for i in range(lcap):
            ml = g.new_line(xyz[i], normal[i], dist[i], 0)
            ml.desc = desc0[i].copy()
            if okh[i]:
                g.observe(ml, 0, i)
            else:
                ml.bad = True
        return g
    g = graph(host(ln["ln_xyz"]), host(ln["ln_normal"]), host(ln["ln_dist"]))
    lst_h = host(cand)[0, :int(n_cand[0])].tolist()
    assert lst_h == [i for i in range(lcap) if okh[i]] and len(lst_h) >= 15
    got = {k: host(v) for k, v in fout.items()}
    stats = dict(REPLACED_BY_HELD=0, REPLACES_HELD=0, SELF=0, researched=0, research_changed=0, UNRESOLVED=0, repeated=0, added_in_kf=0, checked=0)
    entry = DeviceEntry(matcher)
    rets = []
    for f, k in enumerate((1, 2)):
        res = dict({key: got[key][f, :len(lst_h)] for key in ("best_idx", "best_dist", "status", "other")}, _desc=desc0)
        rets.append(lf._replay_item(g, p, entry, g.kfs[k], lst_h, res, True, stats))
        assert rets[-1] == int(got["n_fused"][f])
    live = [ml.id for ml in g.mls if not ml.bad]
    obs = [ml.observations() for ml in g.mls]
    o2 = mappoint.pack_observations(obs)
    flags2 = np.array([0 if ml.bad else 3 for ml in g.mls], np.uint8)          # bit 1: the line has observations (msl_match_local_lines)
    with torch.cuda.stream(s):
        d_o2 = {k: dev(v) for k, v in o2.items()}
        d_flags, d_ids = dev(flags2), dev(np.array(live, np.int32))
        rd = mappoint.refresh_outputs(len(live), zeros=tz)
        r2 = linefuse.refresh_outputs(len(live), zeros=tz)
        mo = torch.full((1, lcap), -7, dtype=torch.int32, device="cuda"); ntm, nm = z(1, torch.int32), z(1, torch.int32)
        dl = [dev(v) for v in larr]
        s.synchronize()
        nobs = int(o2["obs_off"][-1])
        mappoint.refresh_map_points_device(h, rp, 3, klcap, lcap, len(live), nobs, mappoint.REFRESH_DESC,
                                           dict(desc=d_t["ldesc"], n_kps=d_t["n_kl"], kf_flags=torch.ones(3, dtype=torch.uint8, device="cuda")), d_o2,
                                           dict(pt_flags=d_flags), d_ids, rd, dict(pt_desc=ln["ln_desc"]))
        linefuse.refresh_map_lines_device(h, rp, 3, klcap, lcap, len(live), nobs, d_t, d_o2, dict(ln, ln_flags=d_flags), d_ids, r2, ln)
        arrays = dl[:4] + [ln["ln_xyz"], ln["ln_normal"], ln["ln_dist"], ln["ln_desc"], d_flags] + dl[9:]
        h.search_local_lines_device(pll, 1, lcap, lcap, arrays, mo, ntm, nm)
        h.sync()
    # the literal models end to end on the host
    g2 = graph(m["line_xyz"].tolist() + [np.zeros(6)] * (lcap - nk), np.zeros((lcap, 3)), np.zeros((lcap, 2), F32))
    for ml in g2.mls:
        ml.update_average_dir(p)                                               # the MapLine constructor's call
    cands = lf.line_candidates_literal(g2, [0])
    lit = [lf.fuse_literal(p, g2.kfs[k], cands) for k in (1, 2)]
    for ml in g2.mls:
        ml.compute_distinctive_descriptors()
        ml.update_average_dir(p)
    assert lit == rets and sum(lit) >= 25 and g2.snapshot()["slots"] == g.snapshot()["slots"]
    L2 = g2.lines()
    for k, key in (("ln_normal", "normal"), ("ln_dist", "dist"), ("ln_desc", "desc")):
        assert host(ln[k])[live].tobytes() == L2[key][live].tobytes(), k
    assert (L2["nobs"][live] >= 2).sum() >= 10
    local = dict(xyz=L2["xyz"], normal=L2["normal"], dist=L2["dist"], desc=L2["desc"], flags=np.array([0 if ml.bad else 3 for ml in g2.mls], np.uint8))
    wm, wntm, wnm, _, _ = lmm.search_local_lines(pll, cur0, local, Tc[0])
    assert np.array_equal(host(mo)[0, :nk], wm) and int(ntm[0]) == wntm and int(nm[0]) == wnm and wnm >= 10, (host(mo)[0, :nk], wm)
    h.close()

"""msl_fuse_map_points and msl_fuse_candidates on the device against their sequential model (tests/fuse_model.py) on the keyframe graphs of
tests/fuse_scenes.py: every output exactly, the debug accessor's u, v, ur as bytes (the kernels run the model's operations in the model's
order, contraction off; tests/test_fuse_model.py::test_margins keeps every comparison away from its threshold all the same)."""
import numpy as np
import pytest

from tests import fuse_model as fm
from tests import fuse_scenes as fs

pytestmark = pytest.mark.gpu
MSL_ERR_INVALID = -1


def _params(p):
    from manhattanslam_amd import fuse
    return fuse.fuse_params(p["fx"], p["fy"], p["cx"], p["cy"], p["bf"], p["minX"], p["maxX"], p["minY"], p["maxY"], p["scale_factors"],
                            p["inv_level_sigma2"], p["log_scale_factor"], th=p["th"], th_low=p["th_low"])


@pytest.fixture(scope="module")
def matcher():
    from manhattanslam_amd.match import Matcher
    h = Matcher()
    yield h
    h.close()


def _check(got, f, res, n):
    """Item f of the device's outputs against the model's result for a list of n candidates."""
    for k in ("best_idx", "best_dist", "status", "other"):
        assert np.array_equal(got[k][f, :n], res[k]), (f, k, np.flatnonzero(got[k][f, :n] != res[k])[:8], got[k][f, :n][got[k][f, :n] != res[k]][:8],
                                                       np.asarray(res[k])[got[k][f, :n] != res[k]][:8])
    assert int(got["n_fused"][f]) == res["n_fused"], (f, got["n_fused"][f], res["n_fused"])
    # slots beyond the count: -1 for indices, 0 for everything else
    assert (got["best_idx"][f, n:] == -1).all() and (got["other"][f, n:] == -1).all() and not got["best_dist"][f, n:].any() and not got["status"][f, n:].any()
    return res["n_fused"]


def _check_debug(handle, f, res, lcap):
    from manhattanslam_amd import fuse
    d = fuse.debug_fuse(handle, f, lcap)
    n = len(res["trace"])
    for k, dt in (("u", np.float32), ("v", np.float32), ("ur", np.float32), ("level", np.int32), ("n_indices", np.int32)):
        want = np.array([tr[k] for tr in res["trace"]], dt)
        assert d[k][:n].tobytes() == want.tobytes(), (f, k, np.flatnonzero(d[k][:n] != want)[:8])
        assert not d[k][n:].any()


def _ragged():
    """The state of graph a before its second Fuse call, plus a keyframe without keypoints and one with a single keypoint; lists of 0, 1, 63,
    64, 65 and lcap candidates, one of NULLs only, and the current keyframe's own list shared by five targets."""
    table, points, items, res = fs.runs("a")["cand"]
    full = res[0][0]
    own = fs.runs("a")["calls"][0][3][0]
    none = {k: (v[:0] if k != "Tcw" else v) for k, v in table[2].items()}
    one = {k: (v[:1] if k != "Tcw" else v) for k, v in table[3].items()}
    e, o = len(table), len(table) + 1
    table = list(table) + [none, one]
    lists = [[], full[:1], full[:63], full[:64], full[:65], full, [-1] * 10, own[:len(full)]]
    items = [(fs.CUR, l) for l in range(7)] + [(t, 7) for t in (1, 2, 3, 4, 5)] + [(e, 5), (o, 5), (o, 0), (7, 5)]
    return table, points, items, lists


_RAGGED = {}


def _ragged_model():
    if not _RAGGED:
        table, points, items, lists = _ragged()
        _RAGGED["res"] = fm.fuse_map_points(fs.prm(), table, points, items, lists)
    return _RAGGED["res"]


def test_ragged_batch_matches_model(matcher):
    from manhattanslam_amd import fuse
    table, points, items, lists = _ragged()
    lcap = max(len(l) for l in lists)
    cap = max(len(k["kps_un"]) for k in table)
    assert {0, 1, 10, 63, 64, 65, lcap} <= {len(l) for l in lists} and lcap > 100 and {0, 1, cap} <= {len(k["kps_un"]) for k in table}
    got = fuse.fuse_map_points(_params(fs.prm()), table, points, items, lists, handle=matcher)
    assert got["status"].shape == (len(items), lcap)
    res = _ragged_model()
    fused = sum(_check(got, f, res[f], len(lists[l])) for f, (_, l) in enumerate(items))
    assert fused > 60
    assert (got["status"][6, :10] == fm.NULL).all() and (got["best_dist"][6, :10] == 256).all() and got["n_fused"][6] == 0
    assert not got["n_fused"][12] and got["n_fused"][13] <= 2                # no keypoints: nothing fused; one keypoint
    for f, (_, l) in enumerate(items):
        _check_debug(matcher, f, res[f], lcap)


@pytest.mark.parametrize("name", fs.ALL)
def test_coverage_scenes_match_model(matcher, name):
    """Both Fuse calls of SearchInNeighbors on every graph, the first with its seven targets sharing one list."""
    from manhattanslam_amd import fuse
    seen, n = set(), 0
    for table, points, items, lists, res in fs.runs(name)["calls"]:
        if len(lists[0]) == 1:
            continue                                                           # the single-candidate searches of the replay
        got = fuse.fuse_map_points(_params(fs.prm()), table, points, items, lists, handle=matcher)
        for f, (_, l) in enumerate(items):
            _check(got, f, res[f], len(lists[l]))
            _check_debug(matcher, f, res[f], got["status"].shape[1])
            seen |= set(got["status"][f, :len(lists[l])].tolist())
        n += 1
    assert n == 2 and seen == set(range(15))


def test_candidates_match_model(matcher):
    """Overlapping targets, a target named twice, bad points left out, an overflow of lcap with the full count reported, zero targets."""
    from manhattanslam_amd import fuse
    table, points, _, _ = fs.runs("a")["cand"]
    items = [list(fs.TARGETS), [1, 1, 2], [], [3], [2, 1]]
    for lcap in (50, None):
        want = fm.fuse_candidates(table, points, items, lcap=lcap)
        cand, n_cand = fuse.fuse_candidates(table, points, items, handle=matcher, lcap=lcap)
        assert n_cand.tolist() == [n for _, n in want]
        for f, (lst, n) in enumerate(want):
            assert cand[f, :len(lst)].tolist() == lst and (cand[f, len(lst):] == -1).all(), f
    assert n_cand[0] > 50 and n_cand[2] == 0 and n_cand[1] < sum(int((t["held_id"] >= 0).sum()) for t in (table[1], table[2]))
    held_bad = [int(h) for t in fs.TARGETS for h in table[t]["held_id"] if h >= 0 and not points["flags"][h]]
    assert held_bad and not set(held_bad) & set(cand[0].tolist())


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype.names:
        a = a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,))
    return torch.from_numpy(a).cuda()


def _device_call(handle, prm, table, points, items, lists, cap, lcap):
    import torch
    from manhattanslam_amd import fuse
    _, t = fuse.pack_table(table, cap)
    n_pts, p = fuse.pack_points(points)
    _, cand, n_cand = fuse.pack_lists(lists, lcap)
    ins = [_dev(np.array([i[0] for i in items], np.int32)), _dev(np.array([i[1] for i in items], np.int32)), _dev(cand), _dev(n_cand)]
    d_t = {k: _dev(v) for k, v in t.items()}; d_p = {k: _dev(v) for k, v in p.items()}
    out = fuse.outputs(len(items), lcap, zeros=lambda shape, dt: torch.full(shape, 0x5A, dtype=getattr(torch, np.dtype(dt).name), device="cuda"))
    fuse.fuse_map_points_device(handle, prm, len(table), cap, n_pts, len(items), len(cand), lcap, d_t, d_p, *ins, out)
    return out, (d_t, d_p, ins)


def test_memory_paths_and_batch_form_agree(matcher):
    """Host memory on the handle, the _batch form, device memory on the handle's stream and on a caller's stream: the same bytes."""
    import torch
    from manhattanslam_amd import fuse
    from manhattanslam_amd.match import Matcher
    table, points, items, lists, _ = fs.runs("b")["calls"][0]
    prm = _params(fs.prm())
    cap, lcap = max(len(k["kps_un"]) for k in table) + 3, len(lists[0]) + 5
    host = fuse.fuse_map_points(prm, table, points, items, lists, handle=matcher, cap=cap, lcap=lcap)
    batch = fuse.fuse_map_points(prm, table, points, items, lists, cap=cap, lcap=lcap)
    d_out, keep = _device_call(matcher, prm, table, points, items, lists, cap, lcap)
    matcher.sync()
    h2 = Matcher()
    s = torch.cuda.Stream()
    h2.set_stream(s.cuda_stream)
    with torch.cuda.stream(s):
        s_out, keep2 = _device_call(h2, prm, table, points, items, lists, cap, lcap)
        total = s_out["n_fused"].sum()                                        # ordered behind the call by the stream alone
    s.synchronize()
    for k in fuse.OUT_KEYS:
        assert batch[k].tobytes() == host[k].tobytes(), k
        assert d_out[k].cpu().numpy().tobytes() == host[k].tobytes(), k
        assert s_out[k].cpu().numpy().tobytes() == host[k].tobytes(), k
    assert int(total) == int(host["n_fused"].sum()) > 50
    # the candidates: host on the handle, the _batch form, device memory
    tg = [list(fs.TARGETS), [2, 1]]
    c_host, n_host = fuse.fuse_candidates(table, points, tg, handle=matcher, lcap=300)
    c_batch, n_batch = fuse.fuse_candidates(table, points, tg, lcap=300)
    _, t = fuse.pack_table(table)
    n_pts, p = fuse.pack_points(points)
    targets = np.full((2, 7), -1, np.int32); targets[0] = tg[0]; targets[1, :2] = tg[1]
    d = [_dev(x) for x in (t["held_id"], t["n_kps"], p["pt_flags"], targets, np.array([7, 2], np.int32))]
    c_dev = torch.full((2, 300), 0x5A5A5A5A, dtype=torch.int32, device="cuda"); n_dev = torch.zeros(2, dtype=torch.int32, device="cuda")
    fuse.fuse_candidates_device(matcher, len(table), t["held_id"].shape[1], n_pts, 2, 7, 300, *d, c_dev, n_dev)
    matcher.sync()
    assert c_host.tobytes() == c_batch.tobytes() == c_dev.cpu().numpy().tobytes() and n_host.tobytes() == n_batch.tobytes() == n_dev.cpu().numpy().tobytes()
    assert n_host[0] > 100
    h2.close()


def test_limits_are_refused(matcher):
    """Every limit of msl.h, an index outside its table and a list that holds a point twice: MSL_ERR_INVALID, nothing written."""
    from manhattanslam_amd import fuse
    from manhattanslam_amd._lib import lib, ptr
    table, points, items, lists, _ = fs.runs("c")["calls"][0]
    prm = _params(fs.prm())
    cap0, t = fuse.pack_table(table)
    n_pts0, p = fuse.pack_points(points)
    fill = lambda shape, dt: np.full(int(np.prod(shape)) * np.dtype(dt).itemsize, 0x5A, np.uint8).view(dt).reshape(shape)

    def call(cap=cap0, n_tab=len(table), n_pts=n_pts0, n_items=None, lcap=None, prm=prm, items=items, lists=lists):
        lc, cand, n_cand = fuse.pack_lists(lists)
        tgt = np.array([i[0] for i in items], np.int32); lst = np.array([i[1] for i in items], np.int32)
        out = fuse.outputs(len(items), lc, zeros=fill)
        rc = lib.msl_fuse_map_points(matcher.h, n_tab, cap, n_pts, n_items or len(items), len(cand), lcap or lc, ptr(prm), *[ptr(t[k]) for k in fuse.TABLE_KEYS],
                                     *[ptr(p[k]) for k in fuse.POINT_KEYS], ptr(tgt), ptr(lst), ptr(cand), ptr(n_cand), 0,
                                     *[ptr(out[k]) for k in fuse.OUT_KEYS], 0)
        return rc, all((v.view(np.uint8) == 0x5A).all() for v in out.values())

    assert call() == (0, False)
    for kw, word in ((dict(cap=8193), b"cap"), (dict(n_tab=4097), b"n_tab"), (dict(n_pts=1048577), b"n_pts"), (dict(n_items=4097), b"n_items"),
                     (dict(lcap=65537), b"lcap")):
        assert call(**kw) == (MSL_ERR_INVALID, True) and word in lib.msl_last_error(), kw
    for k, v in (("nlevels", 17), ("nlevels", 0), ("th_low", 256), ("th_low", -1)):
        q = prm.copy(); q[k] = v
        assert call(prm=q) == (MSL_ERR_INVALID, True) and k.encode() in lib.msl_last_error(), (k, v)
    own = list(lists[0])
    first = next(x for x in own if x >= 0)
    assert call(lists=[own + [first]]) == (MSL_ERR_INVALID, True) and b"twice" in lib.msl_last_error()
    assert call(lists=[own + [-1, -1]])[0] == 0                               # NULLs may repeat
    assert call(lists=[own + [n_pts0]]) == (MSL_ERR_INVALID, True)
    assert call(lists=[own + [-2]]) == (MSL_ERR_INVALID, True)
    assert call(items=[(len(table), 0)]) == (MSL_ERR_INVALID, True)
    assert call(items=[(-1, 0)]) == (MSL_ERR_INVALID, True)
    assert call(items=[(1, 1)]) == (MSL_ERR_INVALID, True)
    assert call(n_tab=2) == (MSL_ERR_INVALID, True)

    def cands(n_tab=len(table), cap=cap0, n_pts=n_pts0, n_items=1, tcap=7, lcap=64, targets=list(fs.TARGETS), n_targets=7):
        tg = np.array([targets], np.int32); nt = np.array([n_targets], np.int32)
        cand, n_cand = fill((1, 64), np.int32), fill((1,), np.int32)
        rc = lib.msl_fuse_candidates(matcher.h, n_tab, cap, n_pts, n_items, tcap, lcap, ptr(t["held_id"]), ptr(t["n_kps"]), ptr(p["pt_flags"]), ptr(tg),
                                     ptr(nt), 0, ptr(cand), ptr(n_cand), 0)
        return rc, bool((cand.view(np.uint8) == 0x5A).all() and (n_cand.view(np.uint8) == 0x5A).all())

    assert cands() == (0, False)
    for kw, word in ((dict(cap=8193), b"cap"), (dict(n_tab=4097), b"n_tab"), (dict(n_pts=1048577), b"n_pts"), (dict(n_items=4097), b"n_items"),
                     (dict(lcap=65537), b"lcap"), (dict(tcap=65), b"tcap")):
        assert cands(**kw) == (MSL_ERR_INVALID, True) and word in lib.msl_last_error(), kw
    assert cands(targets=[1, 2, 3, 4, 5, 6, len(table)]) == (MSL_ERR_INVALID, True)
    assert cands(n_targets=8) == (MSL_ERR_INVALID, True)


class DeviceEntry(fm.ModelEntry):
    """The two batched entries of the replay on the device (host memory)."""

    def __init__(self, handle):
        fm.ModelEntry.__init__(self)
        self.h = handle

    def candidates(self, table, points, items):
        from manhattanslam_amd import fuse
        cand, n_cand = fuse.fuse_candidates(table, points, items, handle=self.h)
        assert (n_cand <= cand.shape[1]).all()
        return [cand[f, :n_cand[f]].tolist() for f in range(len(items))]

    def fuse(self, prm, table, points, items, lists):
        from manhattanslam_amd import fuse
        got = fuse.fuse_map_points(_params(prm), table, points, items, lists, handle=self.h)
        return [dict({k: got[k][f, :len(lists[l])] for k in ("best_idx", "best_dist", "status", "other")}, n_fused=int(got["n_fused"][f]))
                for f, (_, l) in enumerate(items)]


@pytest.mark.parametrize("name", fs.ALL)
def test_replay_on_device_results(matcher, name):
    """Device search and candidate list, then fuse_model.replay: the graph and the return values of the literal SearchInNeighbors."""
    g, p, cur, targets = fs.graph(name)
    rets, stats = fm.replay(g, p, cur, targets, DeviceEntry(matcher))
    lit_rets, lit_snap = fs.runs(name)["literal"]
    snap = g.snapshot()
    assert rets == lit_rets and snap["slots"] == lit_snap["slots"] and snap["points"] == lit_snap["points"]
    assert stats == fs.runs(name)["replay"][1]


def test_device_chain_triangulate_to_fuse():
    """One stream, no host copy: msl_orb_extract_frame_batch on four frames -> msl_bow_transform -> msl_triangulate_new_points (frame 0 against
    frame 1) -> its item slice as the point table (id = idx1), new_order as the candidate list, pt_flags / pt_nobs by torch ops ->
    msl_fuse_map_points into frames 2 and 3.  The result equals the model run on the copied-back intermediates."""
    import torch
    from manhattanslam_amd import KEYPOINT_DTYPE, ORBextractor, bow, frame_params, fuse, lib, match, synth, triangulate
    from manhattanslam_amd._lib import check, ptr
    from tests import bow_scenes as S
    from tests import bow_model as M
    W, H, B, Z = 320, 240, 4, 2.0
    fx = fy = 260.0; cx, cy, bf = 159.5, 119.5, 5.0
    img0 = np.ascontiguousarray(synth.orb_frame(synth.ORB_SEED + 3)[100:100 + H, 200:200 + W])
    shifts = [(0, 0), (6, -10), (-4, 7), (3, 5)]                              # content moves (down, right) pixels at constant depth
    imgs = np.stack([np.roll(img0, sh, (0, 1)) for sh in shifts]).astype(np.uint8)
    Tcw = np.stack([np.array([[1, 0, 0, sx * Z / fx], [0, 1, 0, sy * Z / fy], [0, 0, 1, 0]], np.float32) for sy, sx in shifts])
    depth = np.full((B, H, W), Z, np.float32)
    fp = frame_params(fx, fy, cx, cy, bf, W, H)
    ex = ORBextractor(400, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=B)
    cap = ex.capacity
    sf, sig2, isig2 = ex.GetScaleFactors(), ex.GetScaleSigmaSquares(), ex.GetInverseScaleSigmaSquares()
    voc = bow.Vocabulary(*S.random_vocab(123, k=10, L=4, scoring=M.L1_NORM, weighting=M.TF_IDF, p_zero=0.02))
    h = match.Matcher()
    s = torch.cuda.Stream()
    check(lib.msl_orb_set_stream(ex._h, s.cuda_stream), "orb stream")
    h.set_stream(s.cuda_stream)
    tp = triangulate.triangulate_params(fx, fy, cx, cy, bf, sf, sig2, 1.2)
    logsf = np.float32(np.log(np.float32(1.2)))
    up = fuse.fuse_params(fx, fy, cx, cy, bf, fp["minX"][0], fp["maxX"][0], fp["minY"][0], fp["maxY"][0], sf, isig2, logsf)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    with torch.cuda.stream(s):
        d_img, d_dep, d_T = _dev(imgs), _dev(depth), _dev(Tcw.reshape(B, 12))
        kps = z((B, cap, 28), torch.uint8); desc = z((B, cap, 32), torch.uint8); un = z((B, cap, 2), torch.float32)
        dp = z((B, cap), torch.float32); ur = z((B, cap), torch.float32); cell = z((B, cap), torch.int32); n = z(B, torch.int32)
        word, node = z((B, cap), torch.int32), z((B, cap), torch.int32)
        held = z((B, cap), torch.uint8)
        cur, neigh, nn = _dev(np.array([0], np.int32)), _dev(np.array([[1]], np.int32)), _dev(np.array([1], np.int32))
        out = triangulate.outputs(1, 1, cap, zeros=lambda shape, dt: z(shape, getattr(torch, np.dtype(dt).name)))
        check(lib.msl_orb_extract_frame_batch(ex._h, ptr(d_img), ptr(d_dep), B, W, H, W, W * H, 4 * W, 4 * W * H, 1, ptr(fp), ptr(kps), ptr(desc),
                                              ptr(un), ptr(dp), ptr(ur), ptr(cell), cap, ptr(n), 1), "orb")
        check(lib.msl_bow_transform(h.h, voc.h, B, cap, 2, ptr(desc), ptr(n), 1, ptr(word), ptr(node), None, None, None, 1), "transform")
        raw = kps.view(torch.float32).reshape(B, cap, 7)[:, :, 0:2].contiguous()      # no distortion: mvKeys = mvKeysUn
        table = dict(kps_un=kps, raw_xy=raw, uright=ur, depth=dp, desc=desc, node=node, held=held, n_kps=n, Tcw=d_T)
        triangulate.triangulate_new_points_device(h, tp, B, cap, 1, 1, table, cur, neigh, nn, out)
        # the item's slice is the point table: id = idx1; a created point is good and has its two observations
        made = out["new_neigh"][0] >= 0
        idx2 = out["new_idx2"][0].clamp(min=0).long()
        obs = (ur[0] >= 0).int() + 1 + (ur[1].index_select(0, idx2) >= 0).int() + 1
        pts = dict(pt_xyz=out["new_xyz"][0], pt_normal=out["new_normal"][0], pt_dist=out["new_dist"][0], pt_desc=out["new_desc"][0],
                   pt_flags=made.to(torch.uint8), pt_nobs=torch.where(made, obs, torch.zeros_like(obs)).contiguous())
        held_id = torch.full((B, cap), -1, dtype=torch.int32, device="cuda")          # only the new points exist: KF1 holds each at its idx1
        held_id[0] = torch.where(made, torch.arange(cap, dtype=torch.int32, device="cuda"), held_id[0])
        ftab = dict(kps_un=kps, uright=ur, grid_cell=cell, desc=desc, n_kps=n, Tcw=d_T, held_id=held_id)
        fout = fuse.outputs(3, cap, zeros=lambda shape, dt: z(shape, getattr(torch, np.dtype(dt).name)))
        tgt, lst = _dev(np.array([2, 3, 0], np.int32)), _dev(np.array([0, 0, 0], np.int32))
        fuse.fuse_map_points_device(h, up, B, cap, cap, 3, 1, cap, ftab, pts, tgt, lst, out["new_order"], out["n_new"], fout)
    s.synchronize()
    # the model on the downloaded intermediates
    nh = n.cpu().numpy()
    kh = kps.cpu().numpy().view(KEYPOINT_DTYPE).reshape(B, cap)
    hid = held_id.cpu().numpy()
    tab = [dict(kps_un=kh[f, :nh[f]], uright=ur[f, :nh[f]].cpu().numpy(), grid_cell=cell[f, :nh[f]].cpu().numpy(), desc=desc[f, :nh[f]].cpu().numpy(),
                Tcw=Tcw[f], held_id=hid[f, :nh[f]]) for f in range(B)]
    points = {k[3:]: v.cpu().numpy() for k, v in pts.items()}
    n_new = int(out["n_new"][0])
    order = out["new_order"][0, :n_new].cpu().numpy().tolist()
    prm = fm.params(fx, fy, cx, cy, bf, fp["minX"][0], fp["maxX"][0], fp["minY"][0], fp["maxY"][0])
    assert prm["scale_factors"].tobytes() == sf.tobytes() and prm["inv_level_sigma2"].tobytes() == isig2.tobytes()
    res = fm.fuse_map_points(prm, tab, points, [(2, 0), (3, 0), (0, 0)], [order])
    got = {k: v.cpu().numpy() for k, v in fout.items()}
    fused = [_check(got, f, res[f], n_new) for f in range(3)]
    assert n_new > 50 and fused[0] > 20 and fused[1] > 20, (n_new, fused)
    assert (got["status"][2, :n_new] == fm.IN_KEYFRAME).all()                # the keyframe that created them holds them all
    h.close(); voc.close(); ex.close()

"""msl_triangulate_new_points on the device against its sequential model (tests/triangulate_model.py) on the fixed scenes of
tests/triangulate_scenes.py: integers and status exactly, the created points as bytes, and the debug accessor's F12, epipole, baseline,
candidates, cosines and homogeneous x3D as bytes (the kernels run the model's operations in the model's order, contraction off;
tests/test_triangulate_model.py::test_margins keeps every decision away from its threshold all the same)."""
import numpy as np
import pytest

from tests import triangulate_model as tm
from tests import triangulate_scenes as ts

pytestmark = pytest.mark.gpu
MSL_ERR_INVALID = -1


def _params(p):
    from manhattanslam_amd import triangulate
    return triangulate.triangulate_params(ts.FX, ts.FY, ts.CX, ts.CY, ts.BF, p["scale_factors"], p["level_sigma2"], 1.2,
                                          check_orientation=p["check_orientation"], only_stereo=p["only_stereo"])


@pytest.fixture(scope="module")
def matcher():
    from manhattanslam_amd.match import Matcher
    h = Matcher()
    yield h
    h.close()


_MODELS = {}


def _model(key, prm, table, items):
    """The model's result per item, computed once per (scene set, switches)."""
    if key not in _MODELS:
        _MODELS[key] = [tm.create_new_map_points(prm, table, c, nb) for c, nb in items]
    return _MODELS[key]


def _check(got, f, res, nb):
    R, n1 = len(nb), len(res["new_neigh"])
    ncap, cap = got["match12"].shape[1:]
    assert np.array_equal(got["match12"][f, :R, :n1], res["match12"]), (f, np.argwhere(got["match12"][f, :R, :n1] != res["match12"])[:8])
    assert np.array_equal(got["status"][f, :R, :n1], res["status"]), (f, np.argwhere(got["status"][f, :R, :n1] != res["status"])[:8])
    assert np.array_equal(got["nmatches"][f, :R], res["nmatches"]), (f, got["nmatches"][f], res["nmatches"])
    for k in ("new_neigh", "new_idx2"):
        assert np.array_equal(got[k][f, :n1], res[k]), (f, k)
    for k in ("new_xyz", "new_normal", "new_dist", "new_desc"):
        assert got[k][f, :n1].tobytes() == res[k].tobytes(), (f, k, np.argwhere(got[k][f, :n1] != res[k])[:8])
    nn = len(res["new_order"])
    assert int(got["n_new"][f]) == nn and np.array_equal(got["new_order"][f, :nn], res["new_order"])
    # slots beyond the counts: -1 for indices, 0 for everything else
    assert (got["match12"][f, R:] == -1).all() and (got["match12"][f, :, n1:] == -1).all() and (got["new_order"][f, nn:] == -1).all()
    assert not got["status"][f, R:].any() and not got["status"][f, :, n1:].any() and not got["nmatches"][f, R:].any()
    assert (got["new_neigh"][f, n1:] == -1).all() and (got["new_idx2"][f, n1:] == -1).all()
    assert not any(got[k][f, n1:].any() for k in ("new_xyz", "new_normal", "new_dist", "new_desc")) and n1 <= cap and R <= ncap
    return nn


def _check_debug(handle, f, res, nb, cap):
    from manhattanslam_amd import triangulate
    n1 = len(res["new_neigh"])
    same = 0
    for r in range(len(nb)):
        d = triangulate.debug_triangulate(handle, f, r, cap)
        tr = res["trace"][r]
        g = tr["geo"]
        assert d["F12"].tobytes() == g["F12"].tobytes(), (f, r, d["F12"], g["F12"])
        assert (d["ex"].tobytes(), d["ey"].tobytes(), d["baseline"].tobytes()) == (g["ex"].tobytes(), g["ey"].tobytes(), g["baseline"].tobytes()), (f, r)
        if tr["skipped"]:
            assert (d["idx2"] == -1).all()
            continue
        c = tr["cand"]
        # the device searches every idx1 from KF1's entry state; the model only those no earlier neighbour has taken
        free = np.ones(n1, bool)
        free[np.nonzero((res["new_neigh"] >= 0) & (res["new_neigh"] < r))[0]] = False
        want = np.full(n1, -1, np.int64); want[c["idx1"]] = c["idx2"]
        assert np.array_equal(d["idx2"][:n1][free], want[free]), (f, r, np.flatnonzero(d["idx2"][:n1][free] != want[free])[:8])
        assert (d["idx2"][n1:] == -1).all()
        assert np.array_equal(d["bin"][c["idx1"]], tr["bins"][c["idx1"]]), (f, r)
        assert d["cos"][c["idx1"]].tobytes() == c["cos"].tobytes(), (f, r, np.argwhere(d["cos"][c["idx1"]] != c["cos"])[:8])
        assert d["x3d"][c["idx1"]].tobytes() == c["x3d"].tobytes(), (f, r, np.argwhere(d["x3d"][c["idx1"]] != c["x3d"])[:8])
        same += len(c["idx1"])
    return same


def _run_scenes(names, handle, key=None, cap_extra=0, ncap=None, **switch):
    from manhattanslam_amd import triangulate
    table, items, _ = ts.combine(names)
    prm = ts.prm(**switch) if switch else ts.scene(names[0])["prm"]
    cap = max(len(k["kps_un"]) for k in table) + cap_extra
    got = triangulate.triangulate_new_points(_params(prm), table, items, handle=handle, cap=cap, ncap=ncap)
    res = _model(key or (names, tuple(sorted(switch.items()))), prm, table, items)
    return table, items, got, res, cap


def _ragged():
    """general + big + special + ring in one table, plus a keyframe without keypoints and one with a single keypoint; items with 0, 1, 3, 10
    and 16 neighbours among them; the largest keyframe fills cap."""
    table, items, _ = ts.combine(("general", "big", "special", "ring"))
    one = {k: (v[:1] if k not in ("Tcw",) else v) for k, v in table[1].items()}
    one["node"] = np.array([int(table[0]["node"][np.flatnonzero(table[0]["node"] >= 0)[0]])], np.int32)
    none = {k: (v[:0] if k not in ("Tcw",) else v) for k, v in table[2].items()}
    none["Tcw"] = ts.make_pose((0.2, -0.3, 0.1), (0.02, 0.0, 0.01))
    e, o = len(table), len(table) + 1
    table = table + [none, one]
    items = items + [(0, []), (0, [o]), (1, [e, 0, o]), (e, [0, 1]), (o, [0])]
    return table, items


def test_ragged_batch_matches_model(matcher):
    from manhattanslam_amd import triangulate
    table, items = _ragged()
    assert sorted({len(nb) for _, nb in items}) == [0, 1, 2, 3, 4, 5, 10, 16]
    cap = max(len(k["kps_un"]) for k in table)
    assert {0, 1, cap} <= {len(k["kps_un"]) for k in table}
    prm = ts.prm(check_orientation=True)
    got = triangulate.triangulate_new_points(_params(prm), table, items, handle=matcher)
    assert got["match12"].shape == (len(items), 16, cap)
    res = _model("ragged", prm, table, items)
    made = sum(_check(got, f, res[f], nb) for f, (_, nb) in enumerate(items))
    cands = sum(_check_debug(matcher, f, res[f], nb, cap) for f, (_, nb) in enumerate(items))
    print("created points:", made, "candidates compared through the debug accessor:", cands)
    assert made > 400 and cands > 400
    seen = set(np.unique(got["status"]).tolist())
    assert seen == set(range(13)) - {tm.W_ZERO, tm.ZERO_DIST}


def test_chain_scene(matcher):
    """The pair (0, 2) as the second neighbour of an item and as a one-neighbour item: both equal the model, and they differ."""
    table, items, got, res, cap = _run_scenes(("chain",), matcher)
    for f, (_, nb) in enumerate(items):
        _check(got, f, res[f], nb)
        _check_debug(matcher, f, res[f], nb, cap)
    n1 = len(table[0]["kps_un"])
    assert (got["match12"][0, 1, :n1] != got["match12"][1, 0, :n1]).any() and got["nmatches"][0, 1] != got["nmatches"][1, 0]


@pytest.mark.parametrize("names,switch", [(("orient",), dict(check_orientation=False)), (("orient",), dict(check_orientation=True)),
                                          (("stereo_only", "general"), dict(only_stereo=True)),
                                          (("special",), dict(only_stereo=True, check_orientation=True))])
def test_switches_and_slots(matcher, names, switch):
    """check_orientation = 0, only_stereo = 1; cap and ncap above every count (the slots beyond are -1 / 0); in every scene a keyframe is the
    current keyframe of one item and a neighbour of another."""
    table, items, got, res, cap = _run_scenes(names, matcher, cap_extra=7, ncap=6, **switch)
    assert any(c in nb2 for c, _ in items for _, nb2 in items)
    made = sum(_check(got, f, res[f], nb) for f, (_, nb) in enumerate(items))
    assert made > 10
    if switch.get("only_stereo"):
        for f, (c, nb) in enumerate(items):
            i = np.flatnonzero(got["new_neigh"][f] >= 0)
            assert (table[c]["uright"][i] >= 0).all()


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype.names:
        a = a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,))
    return torch.from_numpy(a).cuda()


def _device_call(handle, prm, table, items, cap, ncap):
    import torch
    from manhattanslam_amd import triangulate
    _, t = triangulate.pack_table(table, cap)
    _, cur, neigh, n_neigh = triangulate.pack_items(items, ncap)
    tdt = {np.dtype(np.int32): torch.int32, np.dtype(np.uint8): torch.uint8, np.dtype(np.float32): torch.float32}
    d_t = {k: _dev(v) for k, v in t.items()}
    d_out = triangulate.outputs(len(items), ncap, cap, zeros=lambda shape, dt: torch.full(shape, 77, dtype=tdt[np.dtype(dt)], device="cuda"))
    d_cur, d_neigh, d_nn = _dev(cur), _dev(neigh), _dev(n_neigh)
    torch.cuda.synchronize()
    triangulate.triangulate_new_points_device(handle, prm, len(table), cap, len(items), ncap, d_t, d_cur, d_neigh, d_nn, d_out)
    return d_out, (d_t, d_cur, d_neigh, d_nn)


def test_memory_paths(matcher):
    """Host pointers, device pointers (asynchronous on the handle's stream), a caller's stream and the device-indexed form: the same bytes."""
    import torch
    from manhattanslam_amd import triangulate
    from manhattanslam_amd.match import Matcher
    table, items, _ = ts.combine(("special", "orient"))
    prm = _params(ts.prm(check_orientation=True))
    cap, ncap = max(len(k["kps_un"]) for k in table) + 3, 5
    host = triangulate.triangulate_new_points(prm, table, items, handle=matcher, cap=cap, ncap=ncap)
    batch = triangulate.triangulate_new_points(prm, table, items, cap=cap, ncap=ncap)
    d_out, keep = _device_call(matcher, prm, table, items, cap, ncap)
    matcher.sync()
    h2 = Matcher()
    s = torch.cuda.Stream()
    h2.set_stream(s.cuda_stream)
    with torch.cuda.stream(s):
        s_out, keep2 = _device_call(h2, prm, table, items, cap, ncap)
        total = s_out["n_new"].sum()                                          # ordered behind the call by the stream alone
    s.synchronize()
    for k in triangulate.OUT_KEYS:
        assert batch[k].tobytes() == host[k].tobytes(), k
        assert d_out[k].cpu().numpy().tobytes() == host[k].tobytes(), k
        assert s_out[k].cpu().numpy().tobytes() == host[k].tobytes(), k
    assert int(total) == int(host["n_new"].sum()) > 50
    h2.close()


@pytest.fixture(scope="module")
def limit():
    s = ts.limit_scene()
    return s, tm.create_new_map_points(s["prm"], s["table"], *s["items"][0])


def test_cap_8192_is_accepted(matcher, limit):
    """One pair with n = 8192 on both sides, nodes of at most 64 features and one of 1024 (sixteen chunks of the node walk), compared with the
    model chunk by chunk of 1024 idx1."""
    from manhattanslam_amd import triangulate
    s, res = limit
    assert len(s["table"][0]["kps_un"]) == 8192 and np.bincount(s["table"][1]["node"][s["table"][1]["node"] < 1000]).max() == 1024
    got = triangulate.triangulate_new_points(_params(s["prm"]), s["table"], s["items"], handle=matcher)
    assert got["match12"].shape == (1, 1, 8192)
    for a in range(0, 8192, 1024):
        sl = slice(a, a + 1024)
        assert np.array_equal(got["match12"][0, 0, sl], res["match12"][0, sl]), a
        assert np.array_equal(got["status"][0, 0, sl], res["status"][0, sl]), a
        for k in ("new_xyz", "new_normal", "new_dist", "new_desc"):
            assert got[k][0, sl].tobytes() == res[k][sl].tobytes(), (a, k)
    assert _check(got, 0, res, s["items"][0][1]) > 4000
    _check_debug(matcher, 0, res, s["items"][0][1], 8192)


def test_limits_are_refused(matcher):
    """cap = 8193, ncap = 17, nlevels above MSL_MATCH_MAX_LEVELS and a table index out of range: MSL_ERR_INVALID, nothing written."""
    from manhattanslam_amd import triangulate
    from manhattanslam_amd._lib import lib, ptr
    s = ts.scene("chain")
    table = s["table"]
    prm = _params(s["prm"])
    cap0 = max(len(k["kps_un"]) for k in table)

    def call(cap=cap0, ncap=2, p=prm, items=s["items"], n_tab=len(table)):
        _, t = triangulate.pack_table(table, cap0)
        nc, cur, neigh, n_neigh = triangulate.pack_items(items, min(ncap, 16))
        out = triangulate.outputs(len(items), nc, cap0, zeros=lambda shape, dt: np.full(int(np.prod(shape)) * np.dtype(dt).itemsize, 0x5A, np.uint8).view(dt).reshape(shape))
        rc = lib.msl_triangulate_new_points(matcher.h, n_tab, cap, len(items), ncap, ptr(p), *[ptr(t[k]) for k in triangulate.TABLE_KEYS], ptr(cur),
                                            ptr(neigh), ptr(n_neigh), 0, *[ptr(out[k]) for k in triangulate.OUT_KEYS], 0)
        return rc, all((v.view(np.uint8) == 0x5A).all() for v in out.values())

    assert call() == (0, False)
    assert call(cap=8193) == (MSL_ERR_INVALID, True) and b"cap" in lib.msl_last_error()
    assert call(ncap=17) == (MSL_ERR_INVALID, True) and b"ncap" in lib.msl_last_error()
    p17 = prm.copy(); p17["nlevels"] = 17
    assert call(p=p17) == (MSL_ERR_INVALID, True) and b"nlevels" in lib.msl_last_error()
    for bad in ([(3, [1, 2])], [(0, [1, 3])], [(0, [1, -1])], [(0, [1, 1])], [(0, [0, 1])]):     # outside the table, repeated, its own neighbour
        assert call(items=bad) == (MSL_ERR_INVALID, True), bad
    assert call(n_tab=2) == (MSL_ERR_INVALID, True)


def test_device_chain_to_local_points():
    """One stream, no host copy: msl_orb_extract_frame_batch on three frames -> msl_bow_transform -> msl_triangulate_new_points (frame 0
    against frame 1, given poses) -> a torch gather of the created points by new_order -> msl_match_local_points on frame 2.  The result
    equals the two models chained on the downloaded extractor outputs."""
    import torch
    from manhattanslam_amd import KEYPOINT_DTYPE, ORBextractor, bow, frame_params, lib, match, synth, triangulate
    from manhattanslam_amd._lib import check, ptr
    from tests import bow_scenes as S
    from tests import bow_model as M
    from tests import local_match_model as lm
    W, H, B, Z = 320, 240, 3, 2.0
    fx = fy = 260.0; cx, cy, bf = 159.5, 119.5, 5.0
    img0 = np.ascontiguousarray(synth.orb_frame(synth.ORB_SEED + 3)[100:100 + H, 200:200 + W])
    shifts = [(0, 0), (6, -10), (-4, 7)]                                      # content moves (down, right) pixels at constant depth
    imgs = np.stack([np.roll(img0, sh, (0, 1)) for sh in shifts]).astype(np.uint8)
    Tcw = np.stack([np.array([[1, 0, 0, sx * Z / fx], [0, 1, 0, sy * Z / fy], [0, 0, 1, 0]], np.float32) for sy, sx in shifts])
    depth = np.full((B, H, W), Z, np.float32)
    fp = frame_params(fx, fy, cx, cy, bf, W, H)
    ex = ORBextractor(400, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=B)
    cap = ex.capacity
    sf, sig2 = ex.GetScaleFactors(), ex.GetScaleSigmaSquares()
    args = S.random_vocab(123, k=10, L=4, scoring=M.L1_NORM, weighting=M.TF_IDF, p_zero=0.02)
    voc = bow.Vocabulary(*args)
    h = match.Matcher()
    s = torch.cuda.Stream()
    check(lib.msl_orb_set_stream(ex._h, s.cuda_stream), "orb stream")
    h.set_stream(s.cuda_stream)
    tp = triangulate.triangulate_params(fx, fy, cx, cy, bf, sf, sig2, 1.2)
    lp = match.local_match_params(fp, sf, 3.0, np.float32(np.log(np.float32(1.2))))
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    with torch.cuda.stream(s):
        d_img, d_dep, d_T = _dev(imgs), _dev(depth), _dev(Tcw.reshape(B, 12))
        kps = z((B, cap, 28), torch.uint8); desc = z((B, cap, 32), torch.uint8); un = z((B, cap, 2), torch.float32)
        dp = z((B, cap), torch.float32); ur = z((B, cap), torch.float32); cell = z((B, cap), torch.int32); n = z(B, torch.int32)
        word, node = z((B, cap), torch.int32), z((B, cap), torch.int32)
        held = z((B, cap), torch.uint8)
        cur, neigh, nn = _dev(np.array([0], np.int32)), _dev(np.array([[1]], np.int32)), _dev(np.array([1], np.int32))
        out = triangulate.outputs(1, 1, cap, zeros=lambda shape, dt: z(shape, getattr(torch, np.dtype(dt).name)))
        mo, ntm, nm = z((1, cap), torch.int32), z(1, torch.int32), z(1, torch.int32)
        check(lib.msl_orb_extract_frame_batch(ex._h, ptr(d_img), ptr(d_dep), B, W, H, W, W * H, 4 * W, 4 * W * H, 1, ptr(fp), ptr(kps), ptr(desc),
                                              ptr(un), ptr(dp), ptr(ur), ptr(cell), cap, ptr(n), 1), "orb")
        check(lib.msl_bow_transform(h.h, voc.h, B, cap, 2, ptr(desc), ptr(n), 1, ptr(word), ptr(node), None, None, None, 1), "transform")
        raw = kps.view(torch.float32).reshape(B, cap, 7)[:, :, 0:2].contiguous()      # no distortion: mvKeys = mvKeysUn
        table = dict(kps_un=kps, raw_xy=raw, uright=ur, depth=dp, desc=desc, node=node, held=held, n_kps=n, Tcw=d_T)
        triangulate.triangulate_new_points_device(h, tp, B, cap, 1, 1, table, cur, neigh, nn, out)
        order = out["new_order"][0].clamp(min=0).long()                                # slots beyond n_new are not read: n_local = n_new
        mp = [out[k][0].index_select(0, order).unsqueeze(0).contiguous() for k in ("new_xyz", "new_normal", "new_dist", "new_desc")]
        mp_flags = torch.full((1, cap), 3, dtype=torch.uint8, device="cuda")
        check(lib.msl_match_local_points(h.h, 1, cap, cap, ptr(lp), ptr(kps[2:3]), ptr(un[2:3]), ptr(ur[2:3]), ptr(cell[2:3]), ptr(desc[2:3]),
                                         ptr(n[2:3]), ptr(held[2:3]), *[ptr(a) for a in mp], ptr(mp_flags), ptr(out["n_new"]), ptr(d_T[2:3]), 1,
                                         ptr(mo), ptr(ntm), ptr(nm), None, None, 1), "local points")
    s.synchronize()
    # the models on the downloaded extractor and transform outputs
    nh = n.cpu().numpy()
    kh = kps.cpu().numpy().view(KEYPOINT_DTYPE).reshape(B, cap)
    tab = [dict(kps_un=kh[f, :nh[f]], raw_xy=raw[f, :nh[f]].cpu().numpy(), uright=ur[f, :nh[f]].cpu().numpy(), depth=dp[f, :nh[f]].cpu().numpy(),
                desc=desc[f, :nh[f]].cpu().numpy(), node=node[f, :nh[f]].cpu().numpy(), held=np.zeros(nh[f], np.uint8), Tcw=Tcw[f]) for f in range(B)]
    assert np.array_equal(un.cpu().numpy()[0, :nh[0]], tab[0]["raw_xy"])               # the extractor's undistorted points are the keypoints'
    prm = tm.params(fx, fy, cx, cy, bf)
    assert prm["scale_factors"].tobytes() == sf.tobytes() and prm["level_sigma2"].tobytes() == sig2.tobytes()
    res = tm.create_new_map_points(prm, tab, 0, [1])
    got = {k: v.cpu().numpy() for k, v in out.items()}
    made = _check(got, 0, res, [1])
    assert made > 50, made
    o = res["new_order"]
    local = dict(xyz=res["new_xyz"][o], normal=res["new_normal"][o], dist=res["new_dist"][o], desc=res["new_desc"][o], flags=np.full(len(o), 3, np.uint8))
    cur2 = dict(kps=kh[2, :nh[2]], un_xy=un[2, :nh[2]].cpu().numpy(), uright=ur[2, :nh[2]].cpu().numpy(), grid_cell=cell[2, :nh[2]].cpu().numpy(),
                desc=desc[2, :nh[2]].cpu().numpy(), flags=np.zeros(nh[2], np.uint8))
    wm, wntm, wnm, _, _ = lm.search_local_points(lp, cur2, local, Tcw[2])
    assert int(ntm[0]) == wntm and int(nm[0]) == wnm and np.array_equal(mo[0, :nh[2]].cpu().numpy(), wm)
    assert wnm > 20, (wntm, wnm)
    h.close(); voc.close(); ex.close()

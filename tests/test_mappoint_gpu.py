"""msl_refresh_map_points and msl_covisibility on the device against their sequential model (tests/mappoint_model.py) on the scenes of
tests/mappoint_scenes.py.  Every comparison is exact: descriptors, normals and distances as bytes, integers equal (the kernels run the
model's operations in the model's order, contraction off); only the point at a camera centre is compared with a NaN-aware equality."""
import numpy as np
import pytest

from tests import mappoint_model as mm
from tests import mappoint_scenes as ms

pytestmark = pytest.mark.gpu
MSL_ERR_INVALID = -1
SENT = 0xAB
OUT = ("out_desc", "out_normal", "out_dist", "best_obs", "best_median", "status")


@pytest.fixture(scope="module")
def matcher():
    from manhattanslam_amd.match import Matcher
    h = Matcher()
    yield h
    h.close()


def _fill(shape, dt):
    return np.full(int(np.prod(shape)) * np.dtype(dt).itemsize, SENT, np.uint8).view(dt).reshape(shape)


def _rows(n_pts):
    return dict(pt_desc=_fill((n_pts, 32), np.uint8), pt_normal=_fill((n_pts, 3), np.float32), pt_dist=_fill((n_pts, 2), np.float32))


def _refresh(s, handle, ids=None, what=None, rows=None):
    from manhattanslam_amd import mappoint
    rows = _rows(s["n_pts"]) if rows is None else rows
    ids = s["ids"] if ids is None else ids
    got = mappoint.refresh_map_points(mappoint.refresh_params(s["prm"]["scale_factors"]), s["table"], s["obs"], s["points"], ids,
                                      what=s["what"] if what is None else what, rows=rows, handle=handle)
    return got, rows


def _same(a, b, nan_ok=False):
    a, b = np.asarray(a), np.asarray(b)
    if nan_ok:
        return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _check(got, rows, want, ids, nan_items=()):
    """Every per-item output against the model, and the table: the rows of ids hold what was written, every other byte its sentinel."""
    for k in OUT:
        for f in range(len(ids)):
            assert _same(got[k][f], want[k][f], nan_ok=f in nan_items and k == "out_normal"), (k, f, ids[f], got[k][f], want[k][f], got["status"][f])
    expect = _rows(len(rows["pt_desc"]))
    st = want["status"]
    for f, pid in enumerate(ids):
        if st[f] & mm.DESC_WRITTEN:
            expect["pt_desc"][pid] = want["out_desc"][f]
        if st[f] & mm.NORMAL_WRITTEN:
            expect["pt_normal"][pid] = want["out_normal"][f]; expect["pt_dist"][pid] = want["out_dist"][f]
    for k in expect:
        if nan_items and k == "pt_normal":                              # the sentinel is a finite float
            assert np.array_equal(rows[k], expect[k], equal_nan=True), k
        else:
            assert rows[k].tobytes() == expect[k].tobytes(), (k, np.argwhere(rows[k] != expect[k])[:6])


def test_observation_counts(matcher):
    """N = 1 .. 5 (median index 0, 0, 1, 1, 2), the wave edges 63 .. 65, 128, 255, 256, and 257: TOO_MANY with the row untouched."""
    s = ms.counts()
    got, rows = _refresh(s, matcher)
    _check(got, rows, s["want"], s["ids"])
    t = s["tags"]
    assert [len(s["obs"][t["n%d" % n]]) for n in ms.COUNTS] == list(ms.COUNTS)
    for n in ms.COUNTS[:-1]:
        assert got["status"][t["n%d" % n]] == mm.DESC_WRITTEN | mm.NORMAL_WRITTEN
    p = t["n257"]
    assert got["status"][p] == mm.TOO_MANY | mm.NORMAL_WRITTEN and got["best_obs"][p] == -1 and (rows["pt_desc"][p] == SENT).all()
    assert not got["out_desc"][p].any() and np.isfinite(rows["pt_normal"][p]).all()
    assert len({int(got["best_obs"][t["n%d" % n]]) for n in (63, 64, 65, 128, 255, 256)}) > 3      # winners beyond the first lanes' rows
    assert max(int(got["best_obs"][t["n%d" % n]]) for n in (128, 255, 256)) >= 64


def test_special_points(matcher):
    """Ties, bad keyframes, a bad point, no observations, the reference keyframe's place, octaves out of range, a point at a camera centre."""
    s = ms.special()
    t = s["tags"]
    got, rows = _refresh(s, matcher)
    _check(got, rows, s["want"], s["ids"], nan_items=(t["at_centre"], t["at_ref_centre"]))
    both = mm.DESC_WRITTEN | mm.NORMAL_WRITTEN
    st, bo = got["status"], got["best_obs"]
    assert bo[t["tie_later_rows"]] == 1 and bo[t["all_equal"]] == 0 and got["best_median"][t["all_equal"]] == 0
    # bad keyframes: left out of the descriptor, counted in the normal; best_obs is a position in the unfiltered list
    assert st[t["bad_mixed"]] == both and bo[t["bad_mixed"]] in (1, 3, 4, 5) and bo[t["bad_first_of_two"]] == 1
    p = t["all_bad"]
    assert st[p] == mm.NO_LIVE_KF | mm.NORMAL_WRITTEN and (rows["pt_desc"][p] == SENT).all() and np.isfinite(rows["pt_normal"][p]).all()
    for tag, code in (("bad_point", mm.BAD), ("no_obs", mm.NO_OBS)):
        p = t[tag]
        assert st[p] == code and bo[p] == -1 and all((rows[k][p].view(np.uint8) == SENT).all() for k in rows)
        assert not any(got[k][p].any() for k in ("out_desc", "out_normal", "out_dist", "best_median"))
    for tag in ("ref_first", "ref_middle", "ref_last", "ref_absent"):
        assert st[t[tag]] == both, tag
    assert s["points"]["ref"][t["ref_absent"]] not in [k for k, _ in s["obs"][t["ref_absent"]]]
    for tag in ("octave_high", "octave_negative"):
        p = t[tag]
        assert st[p] == mm.DESC_WRITTEN | mm.BAD_OCTAVE and (rows["pt_normal"][p].view(np.uint8) == SENT).all() and (rows["pt_dist"][p].view(np.uint8) == SENT).all()
    assert np.isnan(got["out_normal"][t["at_centre"]]).all() and np.isfinite(got["out_dist"][t["at_centre"]]).all() and got["out_dist"][t["at_centre"]][1] > 0
    assert not got["out_dist"][t["at_ref_centre"]].any()


def test_cross_check_with_triangulation(matcher):
    """The points msl_triangulate_new_points creates: a refresh with their two observations -- KF2 then KF1, KF1 the reference -- gives
    new_desc, new_normal and new_dist again, as bytes."""
    from manhattanslam_amd import mappoint, triangulate
    from tests import triangulate_scenes as ts
    s = ts.scene("general")
    p = s["prm"]
    tp = triangulate.triangulate_params(ts.FX, ts.FY, ts.CX, ts.CY, ts.BF, p["scale_factors"], p["level_sigma2"], 1.2,
                                        check_orientation=p["check_orientation"], only_stereo=p["only_stereo"])
    tri = triangulate.triangulate_new_points(tp, s["table"], s["items"], handle=matcher)
    cap = tri["new_neigh"].shape[1]
    obs, xyz, ref, ids = [], [], [], []
    for f, (k1, nb) in enumerate(s["items"]):
        for i1 in range(cap):
            r = int(tri["new_neigh"][f, i1])
            made = r >= 0
            obs.append([(nb[r], int(tri["new_idx2"][f, i1])), (k1, i1)] if made else [])
            xyz.append(tri["new_xyz"][f, i1]); ref.append(k1)
            if made:
                ids.append(f * cap + i1)
    assert len(ids) > 20
    table = [dict(kps_un=k["kps_un"], desc=k["desc"], Tcw=k["Tcw"]) for k in s["table"]]
    points = dict(flags=np.ones(len(obs), np.uint8), xyz=np.array(xyz, np.float32), ref=np.array(ref, np.int32))
    got = mappoint.refresh_map_points(mappoint.refresh_params(p["scale_factors"]), table, obs, points, ids, handle=matcher)
    assert (got["status"] == mm.DESC_WRITTEN | mm.NORMAL_WRITTEN).all() and (got["best_obs"] == 0).all()
    flat = lambda k: tri[k].reshape((-1,) + tri[k].shape[2:])[ids]
    assert _same(got["out_desc"], flat("new_desc")) and _same(got["out_normal"], flat("new_normal")) and _same(got["out_dist"], flat("new_dist"))


def test_descriptors_alone_over_a_line_table(matcher):
    """MSL_REFRESH_DESC alone: kps_un, Tcw, pt_xyz and pt_ref NULL, normal and distances neither computed nor written."""
    s = ms.lines()
    assert "kps_un" not in s["table"][0] and "xyz" not in s["points"]
    got, rows = _refresh(s, matcher)
    _check(got, rows, s["want"], s["ids"])
    assert (rows["pt_normal"].view(np.uint8) == SENT).all() and (rows["pt_dist"].view(np.uint8) == SENT).all()
    assert {mm.DESC_WRITTEN, mm.NO_OBS} <= set(got["status"].tolist()) <= {mm.DESC_WRITTEN, mm.NO_OBS, mm.NO_LIVE_KF}
    # a geometry scene with DESC alone leaves the geometry alone too; NORMAL alone leaves the descriptors
    c = ms.special()
    for what, untouched in ((mm.REFRESH_DESC, ("pt_normal", "pt_dist")), (mm.REFRESH_NORMAL, ("pt_desc",))):
        want = mm.refresh_map_points(c["prm"], c["table"], c["obs"], c["points"], c["ids"], what)
        got, rows = _refresh(c, matcher, what=what)
        _check(got, rows, want, c["ids"], nan_items=(c["tags"]["at_centre"], c["tags"]["at_ref_centre"]))
        assert all((rows[k].view(np.uint8) == SENT).all() for k in untouched)


@pytest.mark.parametrize("n_items", (1, 64, 65, 5000))
def test_batches(matcher, n_items):
    """Per-item outputs equal the table rows; the rows not named keep their bytes (half of the points are not named)."""
    s = ms.batch()
    ids = s["ids"][:n_items]
    got, rows = _refresh(s, matcher, ids=ids)
    want = {k: v[:n_items] for k, v in s["want"].items()}
    _check(got, rows, want, ids)
    if n_items == 5000:
        assert {len(s["obs"][i]) for i in ids} == set(range(1, 13)) and (got["status"] & mm.NO_LIVE_KF).any()
        named = np.zeros(s["n_pts"], bool); named[ids] = True
        assert (~named).sum() == 5000 and (rows["pt_desc"][~named] == SENT).all()


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype.names:
        a = a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,))
    return torch.from_numpy(a).cuda()


def _packed(s):
    from manhattanslam_amd import mappoint
    cap, t = mappoint.pack_table(s["table"])
    o = mappoint.pack_observations(s["obs"])
    p = dict(pt_xyz=s["points"]["xyz"], pt_flags=s["points"]["flags"], pt_ref=s["points"]["ref"])
    return cap, t, o, p, np.array(s["ids"], np.int32)


def test_memory_paths_and_batch_form_agree(matcher):
    """Host / host on the handle, the _batch form, device / device, and the two mixed forms: the same bytes."""
    from manhattanslam_amd import mappoint
    from manhattanslam_amd._lib import check, lib, ptr
    s = ms.special()
    prm = mappoint.refresh_params(s["prm"]["scale_factors"])
    host, host_rows = _refresh(s, matcher)
    batch, batch_rows = _refresh(s, None)
    cap, t, o, p, ids = _packed(s)
    n_tab, n_pts, F, n_obs = len(s["table"]), s["n_pts"], len(ids), int(o["obs_off"][-1])
    d_in = [_dev(x) for x in [t[k] for k in mappoint.TABLE_KEYS] + [o[k] for k in mappoint.OBS_KEYS] + [p[k] for k in mappoint.POINT_KEYS] + [ids]]
    h_in = [t[k] for k in mappoint.TABLE_KEYS] + [o[k] for k in mappoint.OBS_KEYS] + [p[k] for k in mappoint.POINT_KEYS] + [ids]
    results = []
    for ins, mem, out_mem in ((d_in, 1, 1), (h_in, 0, 1), (d_in, 1, 0)):
        out = mappoint.refresh_outputs(F, zeros=_fill); rows = _rows(n_pts)
        outs = [out[k] for k in mappoint.OUT_KEYS] + [rows[k] for k in mappoint.ROW_KEYS]
        d_outs = [_dev(x) for x in outs] if out_mem else outs
        check(lib.msl_refresh_map_points(matcher.h, n_tab, cap, n_pts, F, n_obs, 3, ptr(prm), *[ptr(x) for x in ins], mem, *[ptr(x) for x in d_outs],
                                         out_mem), "msl_refresh_map_points")
        matcher.sync()
        vals = [x.cpu().numpy() for x in d_outs] if out_mem else outs
        results.append(dict(zip(mappoint.OUT_KEYS + mappoint.ROW_KEYS, vals)))
    nanfree = lambda a: np.where(np.isnan(a), np.float32(7), a) if a.dtype == np.float32 else a
    for r in results + [dict(batch, **batch_rows)]:
        for k in mappoint.OUT_KEYS + mappoint.ROW_KEYS:
            want = host[k] if k in host else host_rows[k]
            assert _same(nanfree(np.asarray(r[k]).reshape(want.shape)), nanfree(want)), k
    # covisibility: host on the handle, the _batch form, device memory
    c = ms.covis_random()
    flags = c["points"]["flags"]
    a = mappoint.covisibility(c["table"], c["obs"], flags, c["kfs"], handle=matcher)
    b = mappoint.covisibility(c["table"], c["obs"], flags, c["kfs"])
    import torch
    cap = max(len(k["held_id"]) for k in c["table"])
    held = np.full((len(c["table"]), cap), -1, np.int32)
    for k, kf in enumerate(c["table"]):
        held[k, :len(kf["held_id"])] = kf["held_id"]
    o = mappoint.pack_observations(c["obs"])
    n_tab = len(c["table"])
    out = mappoint.covisibility_outputs(n_tab, n_tab, n_tab, zeros=lambda sh, dt: torch.full(sh, 0x5A5A5A5A, dtype=torch.int32, device="cuda"))
    mappoint.covisibility_device(matcher, n_tab, cap, len(c["obs"]), n_tab, int(o["obs_off"][-1]), n_tab, 15, _dev(held),
                                 _dev(np.array([len(k["held_id"]) for k in c["table"]], np.int32)), _dev(flags), _dev(o["obs_off"]), _dev(o["obs_kf"]),
                                 _dev(np.array(c["kfs"], np.int32)), out)
    matcher.sync()
    for k in mappoint.COVIS_KEYS:
        assert _same(a[k], b[k]) and _same(a[k], out[k].cpu().numpy()), k


def test_limits_are_refused(matcher):
    """Every limit of msl.h and, with host memory, every defect of the index arrays: MSL_ERR_INVALID, nothing written."""
    from manhattanslam_amd import mappoint
    from manhattanslam_amd._lib import lib, ptr
    s = ms.special()
    prm = mappoint.refresh_params(s["prm"]["scale_factors"])
    cap0, t, o0, p0, ids0 = _packed(s)

    def call(n_tab=len(s["table"]), cap=cap0, n_pts=s["n_pts"], n_items=None, n_obs=None, what=3, prm=prm, o=o0, p=p0, ids=ids0):
        out = mappoint.refresh_outputs(len(ids), zeros=_fill); rows = _rows(s["n_pts"])
        rc = lib.msl_refresh_map_points(matcher.h, n_tab, cap, n_pts, len(ids) if n_items is None else n_items,
                                        int(o["obs_off"][-1]) if n_obs is None else n_obs, what, ptr(prm), *[ptr(t[k]) for k in mappoint.TABLE_KEYS],
                                        *[ptr(o[k]) for k in mappoint.OBS_KEYS], *[ptr(p[k]) for k in mappoint.POINT_KEYS], ptr(ids), 0,
                                        *[ptr(out[k]) for k in mappoint.OUT_KEYS], *[ptr(rows[k]) for k in mappoint.ROW_KEYS], 0)
        return rc, all((v.view(np.uint8) == SENT).all() for v in list(out.values()) + list(rows.values()))

    assert call() == (0, False)
    for kw, word in ((dict(n_tab=4097), b"n_tab"), (dict(n_tab=0), b"n_tab"), (dict(cap=8193), b"cap"), (dict(n_pts=1048577), b"n_pts"),
                     (dict(n_items=s["n_pts"] + 1), b"n_items"), (dict(n_items=0), b"n_items"), (dict(what=0), b"what"), (dict(what=4), b"what"),
                     (dict(n_obs=-1), b"n_obs_total")):
        assert call(**kw) == (MSL_ERR_INVALID, True) and word in lib.msl_last_error(), kw
    for v in (17, 0):
        q = prm.copy(); q["nlevels"] = v
        assert call(prm=q) == (MSL_ERR_INVALID, True) and b"nlevels" in lib.msl_last_error(), v
    # the index arrays (host memory)
    def changed(key, at, value, src=None):
        d = dict(src or o0); d[key] = d[key].copy(); d[key][at] = value
        return d
    some = int(o0["obs_off"][3])
    for o, word in ((changed("obs_off", 2, o0["obs_off"][1] - 1), b"obs_off"), (changed("obs_off", 0, -1), b"obs_off"),
                    (changed("obs_kf", some, len(s["table"])), b"obs_kf"), (changed("obs_kf", some, -1), b"obs_kf"),
                    (changed("obs_idx", some, cap0), b"obs_idx"), (changed("obs_idx", some, -1), b"obs_idx")):
        assert call(o=o) == (MSL_ERR_INVALID, True) and word in lib.msl_last_error(), word
    assert call(n_obs=int(o0["obs_off"][-1]) - 1) == (MSL_ERR_INVALID, True) and b"n_obs_total" in lib.msl_last_error()
    far = int(o0["obs_kf"][some]); idx_far = int(t["n_kps"][far])
    assert call(o=changed("obs_idx", some, idx_far)) == (MSL_ERR_INVALID, True)          # below cap, beyond that keyframe's n_kps
    for ids, word in ((np.array([0, 1, 0], np.int32), b"twice"), (np.array([s["n_pts"]], np.int32), b"ids"), (np.array([-1], np.int32), b"ids")):
        assert call(ids=ids) == (MSL_ERR_INVALID, True) and word in lib.msl_last_error(), word
    bad_ref = dict(p0, pt_ref=p0["pt_ref"].copy()); bad_ref["pt_ref"][2] = len(s["table"])
    assert call(p=bad_ref) == (MSL_ERR_INVALID, True) and b"pt_ref" in lib.msl_last_error()
    assert call(p=bad_ref, ids=np.array([0, 1, 3], np.int32))[0] == 0              # only the items' references are read
    assert call(p=bad_ref, what=1)[0] == 0                                         # and none for descriptors alone

    c = ms.covis_crafted()
    held = np.full((len(c["table"]), 32), -1, np.int32)
    for k, kf in enumerate(c["table"]):
        held[k, :len(kf["held_id"])] = kf["held_id"]
    n_kps = np.array([len(k["held_id"]) for k in c["table"]], np.int32)
    oc = mappoint.pack_observations(c["obs"])
    flags = c["points"]["flags"]

    def covis(n_tab=len(c["table"]), cap=32, n_pts=len(c["obs"]), n_items=2, ccap=4, n_obs=int(oc["obs_off"][-1]), o=oc, kf=(0, 7)):
        kf = np.array(kf, np.int32)
        out = mappoint.covisibility_outputs(2, len(c["table"]), 4, zeros=_fill)
        rc = lib.msl_covisibility(matcher.h, n_tab, cap, n_pts, n_items, n_obs, ccap, 15, ptr(held), ptr(n_kps), ptr(flags), ptr(o["obs_off"]),
                                  ptr(o["obs_kf"]), ptr(kf), 0, *[ptr(out[k]) for k in mappoint.COVIS_KEYS], 0)
        return rc, all((v.view(np.uint8) == SENT).all() for v in out.values())

    assert covis() == (0, False)
    for kw, word in ((dict(n_tab=4097), b"n_tab"), (dict(cap=8193), b"cap"), (dict(n_pts=1048577), b"n_pts"), (dict(n_items=13), b"n_items"),
                     (dict(n_items=0), b"n_items"), (dict(ccap=13), b"ccap"), (dict(ccap=0), b"ccap"), (dict(n_obs=-1), b"n_obs_total"),
                     (dict(kf=(0, 12)), b"kf"), (dict(kf=(-1, 0)), b"kf"), (dict(o=changed("obs_kf", 5, 12, oc)), b"obs_kf"),
                     (dict(o=changed("obs_off", 4, 0, oc)), b"obs_off")):
        assert covis(**kw) == (MSL_ERR_INVALID, True) and word in lib.msl_last_error(), kw
    assert covis(kf=(7, 7))[0] == 0                                                # keyframes may repeat


def _covis_check(got, want):
    for k in ("weight", "conn", "conn_w", "n_conn"):
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])


def test_covisibility_crafted(matcher):
    """Weights 14, 15, 16 around th, ties in the ordered list, the keyframe's own observations, a bad and an out-of-table held id, one point
    in two slots, none >= th with a tie on the maximum, an empty counter, ccap below the count."""
    from manhattanslam_amd import mappoint
    c = ms.covis_crafted()
    flags = c["points"]["flags"]
    got = mappoint.covisibility(c["table"], c["obs"], flags, c["kfs"], handle=matcher)
    _covis_check(got, mm.covisibility(c["table"], c["obs"], flags, c["kfs"]))
    assert got["weight"][0].tolist() == [0, 14, 15, 16, 20, 20, 15, 0, 0, 2, 0, 0]
    assert got["n_conn"].tolist() == [5, 1, 0, 0] and got["conn"][0, :6].tolist() == [5, 4, 3, 6, 2, -1] and got["conn_w"][0, :6].tolist() == [20, 20, 16, 15, 15, 0]
    assert got["conn"][1, :2].tolist() == [8, -1] and got["conn_w"][1, 0] == 3 and got["weight"][1, 8:11].tolist() == [3, 3, 2]
    assert not got["weight"][2:].any() and (got["conn"][2:] == -1).all()
    for th, ccap in ((15, 3), (16, 1), (2, 4), (1, 12), (21, 2)):
        got = mappoint.covisibility(c["table"], c["obs"], flags, c["kfs"], th=th, ccap=ccap, handle=matcher)
        want = mm.covisibility(c["table"], c["obs"], flags, c["kfs"], th, ccap)
        _covis_check(got, want)
        assert got["conn"].shape == (4, ccap)
    assert got["n_conn"][0] == 1 and got["conn"][0, 0] == 4                   # th = 21: none reaches it, the lower index of the two 20s


@pytest.mark.parametrize("n_tab", (1, 2, 30, 4096))
def test_covisibility_table_sizes(matcher, n_tab):
    from manhattanslam_amd import mappoint
    if n_tab <= 2:
        S = ms.Scene(20 + n_tab, n_tab)
        held = {k: [S.point(list(range(n_tab))[::-1] if i % 2 else list(range(n_tab))) for i in range(5)] for k in range(n_tab)}
        c = ms._held(S, held)
        c["kfs"] = list(range(n_tab))
    else:
        c = ms.covis_random() if n_tab == 30 else ms.covis_wide()
    flags = c["points"]["flags"]
    for th in (15, 1):
        got = mappoint.covisibility(c["table"], c["obs"], flags, c["kfs"], th=th, handle=matcher)
        _covis_check(got, mm.covisibility(c["table"], c["obs"], flags, c["kfs"], th))
    if n_tab == 1:
        assert got["n_conn"].tolist() == [0]
    elif n_tab == 2:
        assert got["n_conn"].tolist() == [1, 1] and got["conn"][:, 0].tolist() == [1, 0] and got["conn_w"][:, 0].tolist() == [5, 5]
    elif n_tab == 30:
        assert (got["n_conn"] > 10).all() and (np.diff(got["conn_w"][0, :got["n_conn"][0]]) <= 0).all()
        w = got["conn_w"][0, :got["n_conn"][0]]
        assert (np.diff(w) == 0).any()                                        # equal weights: by descending index
    else:
        assert got["n_conn"].tolist() == [int((got["weight"][0] > 0).sum()), 2, 0] and got["n_conn"][0] > 150
        assert got["conn"][1, :3].tolist() == [0, 4094, -1] and got["conn_w"][1, :3].tolist() == [2, 1, 0]


def test_device_chain_fuse_refresh_match(matcher):
    """SearchInNeighbors on the device entries with the host replay (bookkeeping on the objects; tests/test_fuse_gpu.py), then from one
    upload on without a copy back: the observation table and the flags of the replayed graph -> msl_refresh_map_points for the current
    keyframe's points (src/LocalMapping.cc:573-581) writing into the device point table -> msl_match_local_points of a next frame reading
    that table.  The matches equal the chain of the literal models."""
    import torch
    from manhattanslam_amd import LOCAL_MATCH_PARAMS_DTYPE, fuse, mappoint
    from tests import fuse_model as fm
    from tests import fuse_scenes as fs
    from tests import local_match_model as lm
    from manhattanslam_amd.match import Matcher, pack_local_points
    from tests.test_fuse_gpu import DeviceEntry
    name, nxt = "a", 1
    rprm = mm.params()

    def refs(g):
        for mp in g.mps:
            mp.ref = min(mp.obs) if mp.obs else 0                          # the keyframe that created it; a fusion may take it away

    def frame(g):
        d = g.kfs[nxt].data
        kp = d["kps_un"]
        return dict(kps=kp, un_xy=np.stack([kp["x"], kp["y"]], 1).astype(np.float32), uright=d["uright"], grid_cell=d["grid_cell"], desc=d["desc"],
                    flags=np.zeros(len(kp), np.uint8))

    p = fs.prm()
    lp = np.zeros(1, LOCAL_MATCH_PARAMS_DTYPE)
    for k in ("fx", "fy", "cx", "cy", "bf", "minX", "maxX", "minY", "maxY", "log_scale_factor"):
        lp[k] = p[k]
    lp["th"], lp["nlevels"], lp["view_cos_limit"], lp["nn_ratio"] = 3.0, 8, 0.5, 0.8
    lp["scale_factors"][0, :8] = p["scale_factors"]
    # the model chain: the literal functions on the objects
    g, _, cur, targets = fs.graph(name)
    refs(g)
    fm.search_in_neighbors_literal(g, p, cur, targets)
    mine = [s for s in dict.fromkeys(g.kfs[cur].slots) if s is not None]
    for mp in mine:
        mm.compute_distinctive_descriptors(mp); mm.update_normal_and_depth(mp, rprm)
    pts = g.points()
    local = dict(xyz=pts["xyz"], normal=pts["normal"], dist=pts["dist"], desc=pts["desc"], flags=pts["flags"] | ((pts["nobs"] > 0) * 2).astype(np.uint8))
    want = lm.search_local_points(lp, frame(g), local, g.kfs[nxt].data["Tcw"])
    # the device chain
    g, _, cur, targets = fs.graph(name)
    refs(g)
    fm.replay(g, p, cur, targets, DeviceEntry(matcher))
    ids = [s.id for s in dict.fromkeys(g.kfs[cur].slots) if s is not None]
    assert ids == [m.id for m in mine] and len(ids) > 20
    pts = g.points()                                                       # positions; descriptors, normals, distances as before the refresh
    n_pts = len(g.mps)
    d_rows = dict(pt_desc=_dev(pts["desc"]), pt_normal=_dev(pts["normal"]), pt_dist=_dev(pts["dist"]))
    before = {k: v.clone() for k, v in d_rows.items()}
    cap, t = mappoint.pack_table(mm.graph_table(g))
    o = mappoint.pack_observations(mm.graph_observations(g))
    gp = mm.graph_points(g)
    d_t = {k: _dev(t[k]) for k in mappoint.TABLE_KEYS}; d_o = {k: _dev(v) for k, v in o.items()}
    d_p = dict(pt_xyz=_dev(gp["xyz"]), pt_flags=_dev(gp["flags"]), pt_ref=_dev(gp["ref"]))
    out = mappoint.refresh_outputs(len(ids), zeros=lambda sh, dt: torch.zeros(sh, dtype=getattr(torch, np.dtype(dt).name), device="cuda"))
    h = Matcher()                                                          # a handle of its own on the test's stream
    s = torch.cuda.Stream()
    h.set_stream(s.cuda_stream)
    with torch.cuda.stream(s):
        mappoint.refresh_map_points_device(h, mappoint.refresh_params(rprm["scale_factors"]), len(g.kfs), cap, n_pts, len(ids),
                                           int(o["obs_off"][-1]), 3, d_t, d_o, d_p, _dev(np.array(ids, np.int32)), out, d_rows)
        fr = frame(g)
        fcap, mcap, arrays = pack_local_points([fr], [local], [g.kfs[nxt].data["Tcw"]])
        d_arr = [_dev(a) for a in arrays]
        # the local map is the device point table itself: one frame, mcap = n_pts
        d_arr[7], d_arr[8], d_arr[9], d_arr[10] = d_p["pt_xyz"], d_rows["pt_normal"], d_rows["pt_dist"], d_rows["pt_desc"]
        d_arr[11] = _dev(pts["flags"] | ((pts["nobs"] > 0) * 2).astype(np.uint8))
        match = torch.zeros((1, fcap), dtype=torch.int32, device="cuda"); ntm = torch.zeros(1, dtype=torch.int32, device="cuda")
        nm = torch.zeros(1, dtype=torch.int32, device="cuda")
        h.search_local_points_device(lp, 1, fcap, n_pts, d_arr, match, ntm, nm)
    s.synchronize()
    h.close()
    assert mcap == n_pts
    changed = sum(int((d_rows[k] != before[k]).any(1).sum()) for k in d_rows)
    assert changed > 10                                                    # the refresh did change rows the search then read
    assert np.array_equal(match[0, :len(fr["kps"])].cpu().numpy(), want[0]) and int(ntm[0]) == want[1] and int(nm[0]) == want[2] and want[2] > 10

"""msl_points_3d and msl_keyframe_decision on the device against their sequential model (tests/keyframe_model.py) on the fixed scenes of
tests/keyframe_scenes.py: every output identical as bytes, the slots beyond n_kps included, in the host-memory forms (the handle's and the
device-indexed one) and the device-memory form; the refusals of the handle form; the device-memory contract with guard bands around every
array; and the chain msl_keyframe_decision -> msl_points_3d(enable = need_kf) -> point table -> msl_local_points -> msl_match_local_points
on one stream in device memory against the literal models."""
import re

import numpy as np
import pytest

from tests import keyframe_model as km
from tests import keyframe_scenes as ks

pytestmark = pytest.mark.gpu
MODES = (km.ALL, km.KEYFRAME, km.FRAME)


@pytest.fixture(scope="module")
def matcher():
    from manhattanslam_amd.match import Matcher
    h = Matcher()
    yield h
    h.close()


def _prm():
    from manhattanslam_amd import keyframe
    p = ks.point_params()
    return keyframe.point3d_params(p["fx"], p["fy"], p["cx"], p["cy"], p["th_depth"], p["scale_factors"], p["min_points"])


def _points(frames, mode, cap, handle=None, enable=None, first_id=None, filled=True):
    from manhattanslam_amd import keyframe
    _, a = keyframe.pack_points(list(frames), cap)
    a.update(pt_nobs=ks.table()["pt_nobs"], enable=enable, first_id=first_id)
    out = keyframe.points_outputs(len(frames), cap, ks.host_filled if filled else np.zeros)
    return keyframe.points_3d(_prm(), len(frames), cap, ks.N_PTS, mode, a, out, handle=handle), a


def _sub(model, lo, hi, cap):
    """Frames lo .. hi of a stacked model result, cut to cap slots."""
    return {k: (v[lo:hi, :cap] if v.ndim > 1 else v[lo:hi]).copy() for k, v in model.items()}


def _same(got, want, keys):
    return [k for k in keys if np.asarray(got[k]).tobytes() != np.asarray(want[k]).tobytes()]


@pytest.mark.parametrize("mode", MODES)
def test_ragged_batch_matches_model(matcher, mode):
    """Twelve frames of n_kps 0 .. 4097 in one call: every output, the slots beyond n_kps included."""
    from manhattanslam_amd import keyframe
    got, _ = _points(ks.ragged(), mode, 4097, handle=matcher)
    assert _same(got, ks.point_model("ragged", mode, 4097), keyframe.POINT_OUT_KEYS) == []


@pytest.mark.parametrize("mode", MODES)
def test_full_capacity(matcher, mode):
    """cap = 8192 with every slot a member, 8191 members, and 8192 equal depths (the order is the index order)."""
    from manhattanslam_amd import keyframe
    got, _ = _points(ks.full(), mode, 8192, handle=matcher)
    want = ks.point_model("full", mode, 8192)
    assert _same(got, want, keyframe.POINT_OUT_KEYS) == []
    order = want["new_order"][2, :want["n_new"][2]]
    assert np.all(np.diff(order) > 0) and want["n_new"][2] > 1000 and want["n_walked"][2] == 8192      # all near: the walk never stops
    assert (mode == km.ALL) == (want["n_walked"][0] == 8192) and (mode == km.ALL) == (want["n_walked"][1] == 8191)


def test_enable_and_first_id(matcher):
    """A frame with enable 0 writes its nothing outputs, its neighbours are unaffected; held_out carries first_id + j along new_order."""
    from manhattanslam_amd import keyframe
    enable = tuple(int(f % 3 != 1) for f in range(len(ks.RAGGED)))
    first = np.array([1000 * f + 7 for f in range(len(ks.RAGGED))], np.int32)
    got, a = _points(ks.ragged(), km.KEYFRAME, 4097, handle=matcher, enable=np.array(enable, np.int32), first_id=first)
    assert _same(got, ks.point_model("ragged", km.KEYFRAME, 4097, first=True, enable=enable), keyframe.POINT_OUT_KEYS) == []
    plain = ks.point_model("ragged", km.KEYFRAME, 4097)
    for f, on in enumerate(enable):
        n = int(got["n_new"][f])
        if not on:
            assert n == 0 and got["n_walked"][f] == 0 and not got["pt_new"][f].any() and got["held_out"][f].tobytes() == a["cur_held"][f].tobytes()
            continue
        assert n == plain["n_new"][f] and got["new_xyz"][f].tobytes() == plain["new_xyz"][f].tobytes()
        assert np.array_equal(got["held_out"][f, got["new_order"][f, :n]], first[f] + np.arange(n))


def _decision_inputs(cap, lcap, pcap, only_tracking=0):
    from manhattanslam_amd import keyframe
    t = ks.table()
    _, _, _, a = keyframe.pack_decision(list(ks.decision_frames()), cap, lcap, pcap)
    held, n_kps = ks.table_arrays(cap)
    a.update(pt_nobs=t["pt_nobs"], pt_flags=t["pt_flags"], ln_nobs=t["ln_nobs"], held_id=held, n_kps=n_kps)
    p = ks.DECISION_PARAMS
    return a, keyframe.keyframe_params(p["max_frames"], p["min_frames"], p["th_depth"], only_tracking)


DECISION_SHAPE = (4097, 256, 64)


@pytest.mark.parametrize("only_tracking", [0, 1])
def test_keyframe_decision_matches_model(matcher, only_tracking):
    """The model's scenes as one ragged batch (lines 1, 40, 256; planes 0, 1, 64): every output and both in/out arrays."""
    from manhattanslam_amd import keyframe
    cap, lcap, pcap = DECISION_SHAPE
    a, prm = _decision_inputs(cap, lcap, pcap, only_tracking)
    out = keyframe.decision_outputs(len(ks.decision_frames()), cap, lcap, ks.host_filled)
    keyframe.keyframe_decision(prm, len(ks.decision_frames()), cap, lcap, pcap, ks.N_TAB, ks.N_PTS, ks.N_LINES, a, out, handle=matcher)
    want = ks.decision_expected(cap, lcap, pcap, only_tracking)
    assert _same(dict(out, plane_match=a["plane_match"], plane_outlier=a["plane_outlier"]), want,
                 keyframe.DECISION_OUT_KEYS + keyframe.DECISION_INOUT_KEYS) == []


def test_memory_spaces_and_batch_form(matcher):
    """Host memory, device memory (asynchronous on the handle's stream) and the device-indexed form give the same bytes for both entries;
    NULL enable is every frame, NULL first_id is -1, MSL_POINT3D_ALL reads neither cur_held nor pt_nobs."""
    from manhattanslam_amd import keyframe
    from tests.localmap_scenes import DevArray, device_filled
    frames, cap = ks.ragged()[:10], 257
    F = len(frames)
    host, a = _points(frames, km.FRAME, cap, handle=matcher)
    batch, _ = _points(frames, km.FRAME, cap)
    ones, _ = _points(frames, km.FRAME, cap, handle=matcher, enable=np.ones(F, np.int32))
    d = {k: None if v is None else DevArray(v) for k, v in a.items()}
    dev = keyframe.points_3d_device(matcher, _prm(), F, cap, ks.N_PTS, km.FRAME, d, keyframe.points_outputs(F, cap, device_filled))
    matcher.sync()
    for k in keyframe.POINT_OUT_KEYS:
        assert dev[k].numpy().tobytes() == host[k].tobytes() == batch[k].tobytes() == ones[k].tobytes(), k
        assert dev[k].intact(), k
    assert np.all(host["held_out"][host["pt_new"] == 1] == -1)
    none = dict(a, cur_held=None, pt_nobs=None)
    got = keyframe.points_3d(_prm(), F, cap, 0, km.ALL, none, keyframe.points_outputs(F, cap, ks.host_filled), handle=matcher)
    assert _same(got, _sub(ks.point_model("ragged", km.ALL, 4097), 0, 10, cap), keyframe.POINT_OUT_KEYS) == []
    # msl_keyframe_decision
    cap, lcap, pcap = DECISION_SHAPE
    a, prm = _decision_inputs(cap, lcap, pcap)
    F = len(ks.decision_frames())
    shape = (F, cap, lcap, pcap, ks.N_TAB, ks.N_PTS, ks.N_LINES)
    want = ks.decision_expected(cap, lcap, pcap)
    b = {k: v.copy() for k, v in a.items()}
    batch = keyframe.keyframe_decision(prm, *shape, b, keyframe.decision_outputs(F, cap, lcap, ks.host_filled))
    d = {k: DevArray(v) for k, v in a.items()}
    dev = keyframe.keyframe_decision_device(matcher, prm, *shape, d, keyframe.decision_outputs(F, cap, lcap, device_filled))
    matcher.sync()
    got = {k: v.numpy() for k, v in dev.items()}
    got.update(plane_match=d["plane_match"].numpy(), plane_outlier=d["plane_outlier"].numpy())
    keys = keyframe.DECISION_OUT_KEYS + keyframe.DECISION_INOUT_KEYS
    assert _same(got, want, keys) == [] and _same(dict(batch, plane_match=b["plane_match"], plane_outlier=b["plane_outlier"]), want, keys) == []
    assert all(v.intact() for v in list(dev.values()) + list(d.values()))


def test_refusals(matcher):
    """Each limit exceeded by one: MSL_ERR_INVALID from the handle form with the field named, before any launch -- the outputs keep their
    bytes; the limits themselves are accepted."""
    from manhattanslam_amd import _lib, keyframe
    from tests.test_keyframe_abi import LIMITS
    frames = [ks.point_frame(70, 5), ks.point_frame(71, 3)]
    _, a = keyframe.pack_points(frames, 6)
    a.update(pt_nobs=ks.table()["pt_nobs"], enable=None, first_id=None)
    sh = dict(n_frames=2, cap=6, n_pts=ks.N_PTS, mode=km.KEYFRAME)
    for field, value, msg in LIMITS["msl_points_3d"]:
        out = keyframe.points_outputs(2, 6, ks.host_filled)
        s = dict(sh, **{field: value})
        rc = _lib.lib.msl_points_3d(matcher.h, s["n_frames"], s["cap"], s["n_pts"], s["mode"], _lib.ptr(_prm()), *[_lib.ptr(a[k]) for k in keyframe.POINT_IN_KEYS],
                                    0, *[_lib.ptr(out[k]) for k in keyframe.POINT_OUT_KEYS], 0)
        assert rc == -1 and _lib.lib.msl_last_error().decode() == f"msl_points_3d: {msg}" and all((v.view(np.uint8) == ks.FILL).all() for v in out.values())
    dframes = [ks.decision_frame(70, 5, 2, 1), ks.decision_frame(71, 3, 4, 2)]
    _, _, _, d = keyframe.pack_decision(dframes, 6, 4, 2)
    t = ks.table()
    held, n_kps = ks.table_arrays(6)
    d.update(pt_nobs=t["pt_nobs"], pt_flags=t["pt_flags"], ln_nobs=t["ln_nobs"], held_id=held, n_kps=n_kps)
    sh = dict(n_frames=2, cap=6, lcap=4, pcap=2, n_tab=ks.N_TAB, n_pts=ks.N_PTS, n_lines=ks.N_LINES)
    prm = keyframe.keyframe_params(30, 0, 3.0)
    for field, value, msg in LIMITS["msl_keyframe_decision"]:
        out = keyframe.decision_outputs(2, 6, 4, ks.host_filled)
        with pytest.raises(_lib.MslError, match=re.escape(msg)):
            keyframe.keyframe_decision(prm, *[dict(sh, **{field: value})[k] for k in sh], d, out, handle=matcher)
        assert all((v.view(np.uint8) == ks.FILL).all() for v in out.values())
    # the limits themselves: n_tab 4096, n_pts and n_lines 1 << 20, lcap 256, pcap 64 on small frames (cap 8192 is test_full_capacity's)
    fr = [ks.decision_frame(72, 9, 256, 64, ref_kf=4095)]
    _, _, _, d = keyframe.pack_decision(fr, 9, 256, 64)
    big = np.zeros(1 << 20, np.int32)
    big[:ks.N_PTS] = t["pt_nobs"]
    flags = np.zeros(1 << 20, np.uint8)
    flags[:ks.N_PTS] = t["pt_flags"]
    lines = np.zeros(1 << 20, np.int32)
    lines[:ks.N_LINES] = t["ln_nobs"]
    held = np.full((4096, 9), -1, np.int32)
    held[4095] = fr[0]["cur_held"]
    d.update(pt_nobs=big, pt_flags=flags, ln_nobs=lines, held_id=held, n_kps=np.full(4096, 9, np.int32))
    out = keyframe.keyframe_decision(prm, 1, 9, 256, 64, 4096, 1 << 20, 1 << 20, d, handle=matcher)
    want = km.keyframe_decision(dict(ks.DECISION_PARAMS), fr[0], [np.zeros(0, np.int32)] * 4095 + [fr[0]["cur_held"]], t["pt_nobs"], t["pt_flags"], t["ln_nobs"])
    assert out["counts"][0].tolist() == want["counts"].tolist() and int(out["need_kf"][0]) == want["need_kf"] and int(out["n_inliers"][0]) == want["n_inliers"]
    got = keyframe.points_3d(_prm(), 2, 6, 1 << 20, km.KEYFRAME, dict(a, pt_nobs=big), handle=matcher)
    small, _ = _points(frames, km.KEYFRAME, 6, handle=matcher)
    assert _same(got, small, keyframe.POINT_OUT_KEYS) == []


def test_device_contract_outside_ids_and_counts(matcher):
    """Device memory: an id outside its table counts as NULL, counts are clamped into 0 .. cap, and nothing is written outside the arrays
    (guard bands around every input and output)."""
    from manhattanslam_amd import keyframe
    from tests.localmap_scenes import DevArray, device_filled
    frames, cap = list(ks.ragged()[6:10]), 257                           # 127, 128, 129, 257 slots
    F = len(frames)
    _, a = keyframe.pack_points(frames, cap)
    a["pt_nobs"] = ks.table()["pt_nobs"]
    want = _sub(ks.point_model("ragged", km.KEYFRAME, 4097), 6, 10, cap)
    null = (a["cur_held"] == -1) & (np.arange(cap)[None, :] < a["n_kps"][:, None])   # the NULL slots below n_kps
    odd = np.resize([ks.N_PTS, -7, 1 << 30], int(null.sum())).astype(np.int32)
    a["cur_held"][null] = odd
    keep = null & (want["pt_new"] == 0)                                # held_out keeps the id as it stands where no point is made
    want["held_out"][keep] = a["cur_held"][keep]
    a["n_kps"][3] = cap + 9                                            # a full row: the clamp changes nothing
    a["n_kps"][0] = -5                                                 # no slots at all
    empty = km.points_3d(km.KEYFRAME, ks.point_params(), frames[0]["kps_un"][:0], frames[0]["depth"][:0], frames[0]["desc"][:0], frames[0]["Tcw"],
                         frames[0]["cur_held"][:0], a["pt_nobs"], cap=cap)
    for k in want:
        want[k][0] = empty[k]
    d = {k: DevArray(v) for k, v in a.items()}
    dev = keyframe.points_3d_device(matcher, _prm(), F, cap, ks.N_PTS, km.KEYFRAME, dict(d, enable=None, first_id=None), keyframe.points_outputs(F, cap, device_filled))
    matcher.sync()
    assert _same({k: v.numpy() for k, v in dev.items()}, want, keyframe.POINT_OUT_KEYS) == []
    assert all(v.intact() for v in list(dev.values()) + list(d.values()))
    # msl_keyframe_decision: NULL slots become ids outside the tables, n_cur beyond cap on a full row
    dcap, lcap, pcap = DECISION_SHAPE
    a, prm = _decision_inputs(dcap, lcap, pcap)
    want = ks.decision_expected(dcap, lcap, pcap)
    n_cur, n_lines = a["n_cur"].copy(), a["n_cur_lines"].copy()
    for key, out_key, n, limit in (("cur_held", "held_out", n_cur, ks.N_PTS), ("cur_lheld", "lheld_out", n_lines, ks.N_LINES)):
        live = np.arange(a[key].shape[1])[None, :] < n[:, None]
        null = (a[key] == -1) & live
        a[key][null] = np.resize([limit, -9, 1 << 30], int(null.sum())).astype(np.int32)
        want[out_key][null] = a[key][null]                             # copied as they stand
    null = a["held_id"] == -1
    a["held_id"][null] = np.resize([ks.N_PTS, -2], int(null.sum())).astype(np.int32)
    a["n_cur"][12] = dcap + 1; a["n_cur_lines"][3] = lcap + 4; a["n_planes"][3] = pcap + 1; a["n_kps"][4] = dcap + 100
    want_row4 = a["held_id"][4].copy()
    assert (want_row4[300:] != -1).all()                               # the row's tail now holds ids outside the table: they count as NULL
    F = len(ks.decision_frames())
    d = {k: DevArray(v) for k, v in a.items()}
    dev = keyframe.keyframe_decision_device(matcher, prm, F, dcap, lcap, pcap, ks.N_TAB, ks.N_PTS, ks.N_LINES, d, keyframe.decision_outputs(F, dcap, lcap, device_filled))
    matcher.sync()
    got = {k: v.numpy() for k, v in dev.items()}
    got.update(plane_match=d["plane_match"].numpy(), plane_outlier=d["plane_outlier"].numpy())
    assert _same(got, want, keyframe.DECISION_OUT_KEYS + keyframe.DECISION_INOUT_KEYS) == []
    assert all(v.intact() for v in list(dev.values()) + list(d.values()))


def _chain_scene(B=2, n=200, n_pts0=150):
    """Frame t of every f: keypoints with depths under a random pose, slots that hold points of an existing table (some without
    observations).  Frame t + 1: the camera a little further on; its keypoints are the projections of the points the model creates from
    frame t, with pixel noise, their descriptors noisy copies."""
    from manhattanslam_amd import KEYPOINT_DTYPE
    from tests import local_match_scenes as lms, match_scenes as ms
    p = lms.params()
    prm = km.params(*(float(p[k][0]) for k in ("fx", "fy", "cx", "cy")), th_depth=3.0)
    n_pts = n_pts0 + B * n
    rng = np.random.default_rng(77)
    tab = dict(xyz=rng.normal(0, 3, (n_pts, 3)).astype(np.float32), normal=rng.normal(0, 1, (n_pts, 3)).astype(np.float32),
               dist=np.abs(rng.normal(3, 1, (n_pts, 2))).astype(np.float32), desc=rng.integers(0, 256, (n_pts, 32), dtype=np.uint8),
               flags=(np.arange(n_pts) < n_pts0).astype(np.uint8), nobs=np.where(np.arange(n_pts) < n_pts0, rng.integers(0, 4, n_pts), 0).astype(np.int32))
    frames, nxt, Tn = [], [], []
    for f in range(B):
        kps = np.zeros(n, KEYPOINT_DTYPE)
        xy = np.round(np.stack([rng.uniform(30, 610, n), rng.uniform(30, 450, n)], 1) * 4).astype(np.float32) / 4
        kps["x"], kps["y"], kps["octave"], kps["class_id"] = xy[:, 0], xy[:, 1], rng.integers(0, 8, n), -1
        depth = rng.uniform(0.8, 6.0, n).astype(np.float32)
        depth[rng.random(n) < 0.1] = 0.0
        T = np.eye(4, dtype=np.float32)
        T[:3, :3], T[:3, 3] = lms.rotation(rng, 8.0), rng.normal(0, 0.3, 3)
        held = np.where(rng.random(n) < 0.4, rng.integers(0, n_pts0, n), -1).astype(np.int32)
        fr = dict(ks.RECORD, ref_kf=0, kps_un=kps, depth=depth, desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), Tcw=T[:3].copy(), cur_held=held,
                  outlier=(rng.random(n) < 0.1).astype(np.uint8), cur_lheld=np.zeros(0, np.int32), line_outlier=np.zeros(0, np.uint8),
                  plane_match=np.full((1 - f, 3), -1, np.int32), plane_outlier=np.zeros((1 - f, 3), np.uint8), local_mapping_stopped=f)
        frames.append(fr)
        T1 = T.copy()
        T1[:3, 3] += np.array([0.02, -0.01, 0.03], np.float32)
        Tn.append(T1)
    return p, prm, tab, frames, Tn, n_pts, n_pts0, rng, ms


def test_chain_decision_points_table_local_match():
    """msl_keyframe_decision, msl_points_3d(MSL_POINT3D_KEYFRAME, enable = need_kf) on its cleaned slots, the new rows scattered into the
    device point table at held_out, msl_local_points and msl_match_local_points on the next frame: one handle, one stream, device tensors
    throughout.  The matches equal the literal models'; the new rows equal msl_refresh_map_points over the one-observation table."""
    import torch
    from manhattanslam_amd import keyframe, localmap, mappoint, match
    from tests import local_match_model as lmm, local_match_scenes as lms, localmap_model as lm, mappoint_model as mm
    B, n = 2, 200
    p, prm, tab, frames, Tn, n_pts, n_pts0, rng, ms = _chain_scene(B, n)
    dprm = dict(ks.DECISION_PARAMS)
    kf_row = np.where(rng.random(n) < 0.7, rng.integers(0, n_pts0, n), -1).astype(np.int32)
    # ---- the models in sequence ----
    dec = [km.keyframe_decision(dprm, fr, [kf_row], tab["nobs"][:n_pts0], tab["flags"][:n_pts0], np.zeros(1, np.int32)) for fr in frames]
    assert [d["need_kf"] for d in dec] == [1, 0] and all(d["track_ok"] for d in dec)
    first = np.array([n_pts0 + f * n for f in range(B)], np.int32)
    pts = [km.points_3d(km.KEYFRAME, prm, fr["kps_un"], fr["depth"], fr["desc"], fr["Tcw"], dec[f]["held_out"], tab["nobs"], enable=bool(dec[f]["need_kf"]),
                        first_id=int(first[f])) for f, fr in enumerate(frames)]
    assert pts[0]["n_new"] > 60 and pts[1]["n_new"] == 0 and pts[0]["cleared"].sum() == 0          # the decision cleaned the slots before
    want_tab = {k: v.copy() for k, v in tab.items()}
    for f in range(B):
        for i in pts[f]["new_order"][:pts[f]["n_new"]]:
            r = pts[f]["held_out"][i]
            want_tab["xyz"][r], want_tab["normal"][r], want_tab["dist"][r], want_tab["desc"][r] = (pts[f]["new_" + k][i] for k in ("xyz", "normal", "dist", "desc"))
            want_tab["flags"][r], want_tab["nobs"][r] = 1, 1
    # frame t + 1: the new points of frame 0 (and the old table's of frame 1) seen from a camera a little further on
    cur, want = [], []
    fx, fy, cx, cy, bf = (float(p[k][0]) for k in ("fx", "fy", "cx", "cy", "bf"))
    for f in range(B):
        held = [int(i) if i >= 0 else None for i in pts[f]["held_out"]]
        local = lm.update_local_elements([0], [held], [not x for x in want_tab["flags"]])
        flags = lm.element_flags(local, set(), want_tab["nobs"])
        rows = dict({k: want_tab[k][local] for k in ("xyz", "normal", "dist", "desc")}, flags=np.array(flags, np.uint8))
        T1 = Tn[f].astype(np.float64)
        Pc = (T1[:3, :3] @ want_tab["xyz"][local].astype(np.float64).T).T + T1[:3, 3]
        src = np.array([held.index(q) for q in local])
        zc = np.where(np.abs(Pc[:, 2]) < 1e-3, 1e-3, Pc[:, 2])
        xy = np.stack([fx * Pc[:, 0] / zc + cx, fy * Pc[:, 1] / zc + cy], 1) + rng.normal(0, 0.4, (len(local), 2))
        xy = np.round(np.clip(xy, 1, [638, 478]) * 4).astype(np.float32) / 4
        kps = frames[f]["kps_un"][src].copy()
        kps["x"], kps["y"] = xy[:, 0], xy[:, 1]
        desc = want_tab["desc"][local].copy()
        flip = rng.integers(0, 256, (len(local), 8))
        for k in range(8):
            desc[np.arange(len(local)), flip[:, k] // 8] ^= (1 << (flip[:, k] % 8)).astype(np.uint8)
        c = dict(kps=kps, un_xy=xy, uright=(xy[:, 0] - bf / np.maximum(Pc[:, 2], 0.1)).astype(np.float32), grid_cell=ms.grid_cells(xy, p), desc=desc,
                 flags=np.zeros(len(local), np.uint8))
        cur.append(c)
        want.append((local, lmm.search_local_points(p, c, rows, Tn[f])))
    assert want[0][1][2] > 40 and len(want[0][0]) > 100
    # ---- the device: everything stays there ----
    cap, lcap, pcap = n, 1, 1
    _, _, _, da = keyframe.pack_decision(frames, cap, lcap, pcap)
    da.update(pt_nobs=tab["nobs"], pt_flags=tab["flags"], ln_nobs=np.zeros(1, np.int32), held_id=kf_row[None].copy(), n_kps=np.array([n], np.int32))
    _, pa = keyframe.pack_points(frames, cap)
    _, mcap, ma = match.pack_local_points(cur, [lms.empty_local(dict(xyz=tab["xyz"], normal=tab["normal"], dist=tab["dist"], desc=tab["desc"], flags=tab["flags"]))] * B,
                                          np.stack(Tn), cap, cap)
    h = match.Matcher()
    stream = torch.cuda.Stream()
    h.set_stream(stream.cuda_stream)
    try:
        dev = lambda v: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1)).cuda()
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        with torch.cuda.stream(stream):
            d = {k: dev(v) for k, v in da.items()}
            q = {k: dev(v) for k, v in pa.items()}
            row = lambda v, w: torch.cat([torch.from_numpy(v).cuda(), z((1, w) if w else (1,), torch.from_numpy(v).dtype)]).contiguous()   # and a spare row
            T = dict(pt_xyz=row(tab["xyz"], 3), pt_normal=row(tab["normal"], 3), pt_dist=row(tab["dist"], 2), pt_desc=row(tab["desc"], 32),
                     pt_flags=row(tab["flags"], 0), pt_nobs=row(tab["nobs"], 0))
            d["pt_nobs"] = q["pt_nobs"] = T["pt_nobs"]; d["pt_flags"] = T["pt_flags"]
            do = dict(found_pt=z((B, cap), torch.uint8), found_line=z((B, lcap), torch.uint8), n_inliers=z(B, torch.int32), track_ok=z(B, torch.uint8),
                      new_plane=z(B, torch.uint8), held_out=z((B, cap), torch.int32), outlier_out=z((B, cap), torch.uint8), lheld_out=z((B, lcap), torch.int32),
                      line_outlier_out=z((B, lcap), torch.uint8), counts=z((B, 4), torch.int32), cond=z(B, torch.uint8), need_kf=z(B, torch.int32))
            po = dict(pt_new=z((B, cap), torch.uint8), cleared=z((B, cap), torch.uint8), new_xyz=z((B, cap, 3), torch.float32),
                      new_normal=z((B, cap, 3), torch.float32), new_dist=z((B, cap, 2), torch.float32), new_desc=z((B, cap, 32), torch.uint8),
                      held_out=z((B, cap), torch.int32), new_order=z((B, cap), torch.int32), n_new=z(B, torch.int32), n_walked=z(B, torch.int32))
            lo = dict(local_id=z((B, mcap), torch.int32), n_local=z(B, torch.int32), mp_xyz=z((B, mcap, 3), torch.float32), mp_normal=z((B, mcap, 3), torch.float32),
                      mp_dist=z((B, mcap, 2), torch.float32), mp_desc=z((B, mcap, 32), torch.uint8), mp_flags=z((B, mcap), torch.uint8), cur_flags=z((B, cap), torch.uint8))
            li = dict(local_kf=dev(np.array([[0, -1], [1, -1]], np.int32)), n_local_kf=dev(np.ones(B, np.int32)), n_kps=dev(np.full(B, n, np.int32)),
                      cur_held=dev(np.full((B, cap), -1, np.int32)), n_cur=dev(np.array([len(c["kps"]) for c in cur], np.int32)))
            m = [dev(x) for x in ma]
            mo, ntm, nm = z((B, cap), torch.int32), z(B, torch.int32), z(B, torch.int32)
            stream.synchronize()                                           # the uploads are done; from here on the handle and torch enqueue on one stream
            keyframe.keyframe_decision_device(h, keyframe.keyframe_params(dprm["max_frames"], dprm["min_frames"], dprm["th_depth"]), B, cap, lcap, pcap, 1,
                                              n_pts, 1, d, do)
            keyframe.points_3d_device(h, keyframe.point3d_params(prm["fx"], prm["fy"], prm["cx"], prm["cy"], prm["th_depth"], prm["scale_factors"]), B, cap,
                                      n_pts, km.KEYFRAME, dict(q, cur_held=do["held_out"], enable=do["need_kf"], first_id=dev(first)), po)
            # the new rows into the table at held_out; a slot without a new point writes the spare row n_pts
            idx = torch.where(po["pt_new"].bool(), po["held_out"], torch.full_like(po["held_out"], n_pts)).reshape(-1).long()
            for k in ("xyz", "normal", "dist", "desc"):
                T["pt_" + k].index_copy_(0, idx, po["new_" + k].reshape(B * cap, -1))
            T["pt_flags"].index_fill_(0, idx, 1); T["pt_nobs"].index_fill_(0, idx, 1)
            localmap.local_points_device(h, B, B, cap, n_pts, mcap, dict(li, held_id=po["held_out"], **T), lo)
            h.search_local_points_device(p, B, cap, mcap, m[:6] + [lo[k] for k in ("cur_flags", "mp_xyz", "mp_normal", "mp_dist", "mp_desc", "mp_flags", "n_local")] + [m[-1]],
                                         mo, ntm, nm)
            # the same rows from msl_refresh_map_points over the one-observation table: keyframe f observes point first[f] + j at slot new_order[j]
            n0 = int(pts[0]["n_new"])
            ids = dev(np.arange(n_pts0, n_pts0 + n0, dtype=np.int32))
            obs = dict(obs_off=dev(np.concatenate([np.zeros(n_pts0, np.int32), np.arange(n0 + 1, dtype=np.int32), np.full(n_pts - n_pts0 - n0, n0, np.int32)])),
                       obs_kf=dev(np.zeros(n0, np.int32)), obs_idx=po["new_order"])
            ro = dict(out_desc=z((n0, 32), torch.uint8), out_normal=z((n0, 3), torch.float32), out_dist=z((n0, 2), torch.float32), best_obs=z(n0, torch.int32),
                      best_median=z(n0, torch.int32), status=z(n0, torch.uint8))
            mappoint.refresh_map_points_device(h, mappoint.refresh_params(prm["scale_factors"]), 1, cap, n_pts, n0, n0, 3,
                                               dict(kps_un=q["kps_un"], desc=q["desc"], n_kps=q["n_kps"], Tcw=q["Tcw"], kf_flags=dev(np.ones(1, np.uint8))), obs,
                                               dict(pt_xyz=T["pt_xyz"], pt_flags=T["pt_flags"], pt_ref=z(n_pts + 1, torch.int32)), ids, ro, {})
            h.sync()
        host = lambda t, dt: t.cpu().numpy().view(dt)
        assert host(do["need_kf"], np.int32).tolist() == [1, 0]
        for f in range(B):
            assert host(po["held_out"], np.int32).reshape(B, cap)[f].tobytes() == pts[f]["held_out"].tobytes(), f
            local, (wm, wntm, wnm) = want[f][0], want[f][1][:3]
            nl = len(local)
            assert int(host(lo["n_local"], np.int32)[f]) == nl and host(lo["local_id"], np.int32).reshape(B, mcap)[f, :nl].tolist() == local
            assert np.array_equal(host(mo, np.int32).reshape(B, cap)[f, :len(wm)], wm) and (int(host(ntm, np.int32)[f]), int(host(nm, np.int32)[f])) == (wntm, wnm), f
        for k in ("xyz", "normal", "dist", "desc", "flags", "nobs"):
            assert T["pt_" + k].cpu().numpy()[:n_pts].tobytes() == want_tab[k].tobytes(), k
        order = pts[0]["new_order"][:n0]
        for k in ("desc", "normal", "dist"):
            assert ro["out_" + k].cpu().numpy().tobytes() == pts[0]["new_" + k][order].tobytes(), k
        st = ro["status"].cpu().numpy()
        assert np.all((st & mm.DESC_WRITTEN) != 0) and np.all(((st & mm.NORMAL_WRITTEN) != 0) | ((st & mm.BAD_OCTAVE) != 0))
    finally:
        h.close()

"""msl_keyframe_planes and msl_manhattan_observe on the device against their sequential model (tests/kfplanes_model.py) on the ragged batch of
tests/kfplanes_scenes.py (0, 1, 2, 3, 5 and 12 planes; the cases are listed there): every in/out array and every output identical as bytes,
in both modes, in the host-memory forms (the handle's and the device-indexed one) and the device-memory form under guard bands, where the
rows beyond the counts keep their bytes; the new rows' mp_w equal msl_plane_associate's pM_out and the written keyframe rows what
plane.pack_manhattan builds; the results do not depend on the run or on the composition of the batch; a dot product equal to the
threshold does not pass the gate; and the chain across a keyframe on one
stream in device memory, which ends in a Manhattan frame msl_manhattan_detect can only find in the tables the chain itself wrote."""
import numpy as np
import pytest

from tests import kfplanes_model as kp
from tests import kfplanes_scenes as ks

pytestmark = pytest.mark.gpu
CAPS = (ks.PCAP, ks.MCAP, ks.FCAP, ks.QCAP, ks.KCAP)


@pytest.fixture(scope="module")
def matcher():
    from manhattanslam_amd.match import Matcher
    h = Matcher()
    yield h
    h.close()


@pytest.fixture(scope="module")
def batch():
    from manhattanslam_amd import kfplanes
    return kfplanes.pack(ks.ragged(), *CAPS)[1]


def _params(th=ks.TH):
    from manhattanslam_amd import plane
    return plane.plane_params(0.2, 0.9, 0.08, 0.9, th)


def run(a, mode, form, handle=None, caps=CAPS, th=ks.TH):
    """Both entries on copies of the packed arrays `a`: form "host" (the handle, host memory), "batch" (the device-indexed form, host memory)
    or "device" (the handle, device memory under guard bands; the outputs hold FILL before).  Returns (arrays after, planes outputs, observe
    outputs) as numpy arrays and, for "device", whether every guard band is intact."""
    from manhattanslam_amd import kfplanes
    from tests.localmap_scenes import DevArray, device_filled
    pcap, mcap, fcap, qcap, kcap = caps
    F = len(a["n_planes"])
    dev = form == "device"
    d = {k: DevArray(v) if dev else v.copy() for k, v in a.items()}
    zeros = device_filled if dev else ks.host_filled
    h = None if form == "batch" else handle
    po = kfplanes.keyframe_planes(F, pcap, mcap, kcap, mode, d, kfplanes.planes_outputs(F, pcap, zeros), int(dev), handle=h)
    d["kf_plane_match"] = po["kf_plane_match"]
    oo = kfplanes.manhattan_observe(_params(th), F, pcap, mcap, fcap, qcap, kcap, d, kfplanes.observe_outputs(F, pcap, zeros), int(dev), handle=h)
    if not dev:
        return d, po, oo, True
    handle.sync()
    intact = all(v.intact() for x in (d, po, oo) for v in x.values())
    return ({k: v.numpy() for k, v in d.items()}, {k: v.numpy() for k, v in po.items()}, {k: v.numpy() for k, v in oo.items()}, intact)


def differences(got, want, n_planes, whole):
    """The names whose bytes differ; whole: the rows at and beyond n_planes are compared too (device memory keeps them, a host-memory output
    is copied back whole and is unspecified there)."""
    bad = []
    for g, w in zip(got, want):
        for k in w:
            x, y = np.asarray(g[k]), np.asarray(w[k])
            if not whole and k in ("kf_plane_match", "plane_new", "obs_add", "merge_into", "status", "recent_plane") and x.ndim > 1:
                x, y = x.copy(), y.copy()
                for f, n in enumerate(n_planes):
                    x[f, n:], y[f, n:] = 0, 0
            if x.shape != y.shape or x.tobytes() != y.tobytes():
                bad.append(k)
    return bad


@pytest.mark.parametrize("mode", [kp.KEYFRAME, kp.INIT])
@pytest.mark.parametrize("form", ["host", "batch", "device"])
def test_ragged_batch_matches_model(matcher, batch, mode, form):
    want = ks.expected(batch, mode, fill=ks.host_filled)
    *got, intact = run(batch, mode, form, matcher)
    got[0].pop("kf_plane_match")
    assert differences(got, want, batch["n_planes"], form == "device") == [] and intact
    if mode == kp.INIT:                                                        # every plane a new row while mcap lasts, the frame holds it
        on = batch["frames"]["enable"] != 0
        assert all((got[1]["status"][f, :n] >= kp.NEW).all() for f, n in enumerate(batch["n_planes"]) if on[f])
        assert (got[0]["plane_match"][1, 0, 0], got[1]["status"][5, :12].tolist().count(kp.NO_ROOM)) == (4, 2)


def test_new_rows_are_plane_associate_s_world_coefficients_and_the_keyframe_rows_pack_manhattan_s(matcher, batch):
    from manhattanslam_amd import plane
    from tests import plane_scenes
    frames = ks.ragged()
    a, po, _, _ = run(batch, kp.KEYFRAME, "host", matcher)
    res = plane.plane_association_batch(plane.plane_params(**plane_scenes.PARAMS), frames, handle=matcher, caps=(ks.PCAP, ks.MCAP, 1))
    made = 0
    for f, fr in enumerate(frames):
        for k in range(len(fr["plane_coef"])):
            if po["plane_new"][f, k]:
                made += 1
                row = po["merge_into"][f, k]
                assert row == po["kf_plane_match"][f, k, 0] >= len(fr["mp_w"]) and a["mp_w"][f, row].tobytes() == res[f]["pM"][k].tobytes()
                assert a["mp_flags"][f, row] == 1 and a["mp_first_kf"][f, row] == fr["kf_id"]
    assert made == 3
    for fr in frames:                                                          # the KeyFrame's row as the caller would have built it
        if fr["enable"]:
            s = fr["kf_slot"]
            fr["kf_Rwc"][s] = fr["Tcw"].reshape(3, 4)[:, :3].T.reshape(9)
            fr["kf_coef"][s], fr["kf_npts"][s] = fr["plane_coef"], fr["plane_npts"]
    _, m = plane.pack_manhattan(frames, *CAPS)
    assert a["kf_Rwc"].tobytes() == m[10].tobytes() and a["kf_coef"].tobytes() == m[11].tobytes() and a["kf_npts"].tobytes() == m[12].tobytes()


def test_results_do_not_depend_on_the_run_or_the_batch(matcher, batch):
    first = run(batch, kp.KEYFRAME, "device", matcher)
    again = run(batch, kp.KEYFRAME, "device", matcher)
    assert differences(again[:3], first[:3], batch["n_planes"], True) == []
    order = [8, 3, 5, 0, 7]
    sub = {k: v[order].copy() for k, v in batch.items()}
    got = run(sub, kp.KEYFRAME, "device", matcher)
    want = [{k: v[order] for k, v in x.items()} for x in first[:3]]
    assert differences(got[:3], want, sub["n_planes"], True) == [] and got[3]
    one = {k: v[5:6].copy() for k, v in batch.items()}                         # n_frames = 1
    got = run(one, kp.KEYFRAME, "batch")
    assert differences(got[:3], [{k: v[5:6] for k, v in x.items()} for x in first[:3]], one["n_planes"], False) == []


def test_device_memory_counts_and_indices_outside_their_tables(matcher, batch):
    """What a host-memory call refuses, device memory survives: counts are clamped, a held plane outside the map is NULL, a keyframe row
    outside the table switches the frame off; nothing is written outside an array."""
    a = {k: v.copy() for k, v in batch.items()}
    a["n_planes"][3], a["n_map"][3] = ks.PCAP + 50, -4                         # 13 planes over no map: every plane new
    a["plane_match"][4, 0, 0], a["plane_match"][4, 3, 1] = ks.MCAP + 7, -9
    a["frames"]["kf_slot"][5], a["frames"]["kf_slot"][2] = ks.KCAP, -1
    a["n_full"][1], a["n_part"][1] = -3, ks.QCAP + 9
    want = ks.expected(a, kp.KEYFRAME, fill=ks.host_filled)
    *got, intact = run(a, kp.KEYFRAME, "device", matcher)
    got[0].pop("kf_plane_match")
    assert differences(got, want, a["n_planes"], True) == [] and intact
    assert want[1]["n_new"][3] == ks.PCAP and want[0]["n_map"][3] == ks.PCAP and want[1]["status"][4, 0] == kp.NEW
    assert want[2]["added_full"][5] == 0 and want[0]["kf_Rwc"][5].tobytes() == a["kf_Rwc"][5].tobytes()


def test_a_dot_product_equal_to_the_threshold_is_not_vertical_on_the_device(matcher):
    """Two held planes with the coefficients (1, 0, 0) and (x, 1, 0), whose dot product is x exactly: x = +-th adds no pair, the float next
    to it towards zero adds one (src/LocalMapping.cc:192 compares with < and >)."""
    from manhattanslam_amd import kfplanes
    th = np.float32(ks.TH)
    below = np.nextafter(th, np.float32(0))
    rng = np.random.default_rng(9400)
    frames = []
    for x in (th, -th, below, -below):
        f = ks.frame(rng, 2, 2)
        f["plane_coef"][:, :3] = [[1, 0, 0], [x, 1, 0]]
        f["plane_match"][:, 0] = [0, 1]
        frames.append(f)
    a = kfplanes.pack(frames, *CAPS)[1]
    want = ks.expected(a, kp.KEYFRAME, fill=ks.host_filled)
    assert want[2]["added_part"].tolist() == [0, 0, 1, 1]
    *got, intact = run(a, kp.KEYFRAME, "device", matcher)
    got[0].pop("kf_plane_match")
    assert differences(got, want, a["n_planes"], True) == [] and intact and got[2]["added_part"].tolist() == [0, 0, 1, 1]


def _chain_scene():
    """Four walls seen by one camera (three mutually perpendicular, the fourth parallel to the second), a map that holds the first two and
    a distractor, empty Manhattan tables, and a point / line frame at the same pose whose translation margins pass."""
    from tests import manhattan_model as mh
    from tests import plane_cloud_model as pcm
    from tests import plane_cloud_scenes as pcs
    from tests import plane_match_model as pmm
    from tests import plane_scenes
    from tests import pose_scenes as ps
    from tests import translation_scenes as ts
    pf = pcs.Frame(9300, False)
    for n, c in (((0.02, 0.01, 1.0), (0.0, 0.0, 2.5)), ((1.0, 0.02, -0.01), (-1.5, 0.0, 2.5)), ((0.01, 1.0, 0.02), (0.0, 1.2, 2.5)),
                 ((1.0, 0.03, 0.0), (1.6, 0.0, 2.6))):
        pf.add(pcs.wall(pf.rng, n, c, (0.9, 0.9), 500), n, c)
    cf = pf.done()
    pcap, fptcap = 6, 4096
    want = pcm.plane_clouds(cf, pcs.PRM, pcap, fptcap)
    K = want["n_out"]
    assert K == 4
    clouds = [want["pts"][want["pt_off"][k]:want["pt_off"][k + 1]] for k in range(K)]
    aprm, c = plane_scenes.params(), ps.params()
    seed = 9300
    while True:                                                               # a point scene whose margins pass with these planes
        seed += 1
        fr, _, _ = ps.scene(seed, n_pts=600, n_lines=8, n_planes=0, margin=None, c=c)
        Tcw = np.asarray(fr["Tcw"], np.float32).reshape(12)
        Twc = kp.pose_inverse(Tcw)[1]
        mp_clouds = [pcm.voxel_grid(pcm.transform(Twc, clouds[k])[::2], None, 0.2)[1] for k in range(2)] + [pcs.block(2, 2, 1, (40, 40, 40))]
        mp_w = np.array([pmm.world_coef(Tcw, want["plane_coef"][k]) for k in range(2)] + [[0.0, 0.0, 1.0, -8.1]], np.float32)
        afr = dict(plane_coef=want["plane_coef"], plane_npts=want["plane_npts"], Tcw=Tcw, plane_match=np.full((K, 3), -1, np.int32), mp_w=mp_w,
                   mp_flags=np.ones(3, np.uint8), mp_clouds=mp_clouds)
        n1, match1, _ = pmm.search_map_by_coefficients(afr, aprm)
        if n1 != 2 or match1[:, 0].tolist() != [0, 1, -1, -1]:
            continue
        w, h = pmm.pose_layout(np.array([[0, -1, -1], [1, -1, -1], [3, -1, -1], [4, -1, -1]], np.int32),
                               np.array([pmm.world_coef(Tcw, x) for x in want["plane_coef"][[0, 1, 0, 2, 3]]], np.float32))
        tf = dict(fr, plane_coef=want["plane_coef"], plane_w=w[:, 0:4], par_w=w[:, 4:8], ver_w=w[:, 8:12], plane_has=h & 1, par_has=(h >> 1) & 1,
                  ver_has=(h >> 2) & 1, plane_outlier=np.zeros(K, np.uint8), par_outlier=np.zeros(K, np.uint8), ver_outlier=np.zeros(K, np.uint8))
        try:
            ts.check_margin(tf, c, Tcw.reshape(3, 4)[:, :3].reshape(9))
        except AssertionError:
            continue
        return dict(cf=cf, want=want, clouds=clouds, afr=afr, match1=match1, fr=fr, c=c, aprm=aprm, pcap=pcap, fptcap=fptcap, mh=mh)


def test_chain_across_a_keyframe_on_one_stream_in_device_memory():
    """Frame t: msl_plane_clouds -> msl_plane_associate -> msl_keyframe_decision -> msl_keyframe_planes (enable = need_kf, one tensor copy)
    -> msl_map_plane_merge (its merge_into / Twc) -> msl_manhattan_observe; frame t + 1: msl_plane_associate -> msl_manhattan_detect ->
    msl_pose_optimize_translation.  Two copies of the frame: local mapping takes the keyframe of the first and refuses the second's.  After
    the upload nothing returns to the host until the end.  The chain equals the models chained (bytes; Rcw and Tcw_out within the
    tolerances of their own tests), and the Manhattan frame found at t + 1 is one of keyframe t, which no table held before."""
    import torch
    from manhattanslam_amd import keyframe, kfplanes, plane, plane_cloud, pose
    from manhattanslam_amd.match import Matcher
    from tests import keyframe_model as km
    from tests import plane_cloud_model as pcm
    from tests import plane_cloud_scenes as pcs
    from tests import plane_match_model as pmm
    from tests import translation_model as tm
    S = _chain_scene()
    want, afr, c, aprm, mh, pcap, fptcap = S["want"], S["afr"], S["c"], S["aprm"], S["mh"], S["pcap"], S["fptcap"]
    K, B, mcap, ptcap, fcap, qcap, kcap, slot, kf_id = 4, 2, 8, 8192, 16, 16, 3, 1, 11
    # ---- the models, chained ----
    rec = [dict(flags=km.TRACK_OK, frame_id=40, last_keyframe_id=35, last_reloc_frame_id=0, n_kfs=5, ref_kf=0, n_inliers_in=200,
                local_mapping_idle=idle, local_mapping_stopped=0, keyframes_in_queue=3) for idle in (1, 0)]
    dprm = dict(max_frames=30, min_frames=0, th_depth=3.0, only_tracking=0)
    empty = dict(depth=np.zeros(0, np.float32), cur_held=np.zeros(0, np.int32), outlier=np.zeros(0, np.uint8), cur_lheld=np.zeros(0, np.int32),
                 line_outlier=np.zeros(0, np.uint8), plane_match=S["match1"], plane_outlier=np.zeros((K, 3), np.uint8))
    dec = [km.keyframe_decision(dprm, dict(r, **empty), [np.full(1, -1, np.int32)], np.zeros(1, np.int32), np.zeros(1, np.uint8), np.zeros(1, np.int32))
           for r in rec]
    assert [d["need_kf"] for d in dec] == [1, 0] and all(d["new_plane"] == 1 for d in dec)
    rng = np.random.default_rng(5)
    frames = [dict(afr, enable=d["need_kf"], kf_slot=slot, kf_id=kf_id, plane_match=d["plane_match"], plane_outlier=d["plane_outlier"],
                   mp_first_kf=np.array([2, 2, 4], np.int32), full=np.zeros((0, 7), np.int32), part=np.zeros((0, 5), np.int32),
                   kf_Rwc=rng.normal(size=(kcap, 9)).astype(np.float32), kf_coef=[rng.normal(size=(pcap, 4)).astype(np.float32) for _ in range(kcap)],
                   kf_npts=[rng.integers(1, 9, pcap).astype(np.int32) for _ in range(kcap)]) for d in dec]
    _, a0 = kfplanes.pack(frames, pcap, mcap, fcap, qcap, kcap)
    a, po, oo = ks.expected(a0, kp.KEYFRAME, aprm["mf_ver_th"])
    assert po["status"][0, :K].tolist() == [kp.HELD, kp.HELD, kp.NEW, kp.NEW] and a["n_map"].tolist() == [5, 3] and oo["added_full"].tolist() == [2, 0]
    model = []
    for f in range(B):
        M = int(a["n_map"][f])
        merged = pcm.map_plane_merge(dict(clouds=S["clouds"], rgbs=None, merge_into=po["merge_into"][f, :K].tolist(), Twc=po["Twc"][f],
                                          mp_clouds=afr["mp_clouds"] + [np.zeros((0, 3), np.float32)] * (M - 3), mp_rgbs=None), pcs.PRM, ptcap)
        nxt = dict(afr, plane_match=np.full((K, 3), -1, np.int32), mp_w=a["mp_w"][f, :M], mp_flags=a["mp_flags"][f, :M], mp_clouds=merged["clouds"])
        n2, match2, _ = pmm.search_map_by_coefficients(nxt, aprm)
        mf = dict(nxt, plane_match=match2, full=a["full_tab"][f, :a["n_full"][f]], part=a["part_tab"][f, :a["n_part"][f]], kf_Rwc=a["kf_Rwc"][f],
                  kf_coef=list(a["kf_coef"][f]), kf_npts=list(a["kf_npts"][f]))
        rcw0 = afr["Tcw"].reshape(3, 4)[:, :3].reshape(9)
        found, full, R, cand = mh.detect_manhattan(mf, aprm["mf_ver_th"], rcw0)
        model.append(dict(merged=merged, n2=n2, match2=match2, found=found, full=full, R=R, cand=cand, M=M))
    assert (model[0]["found"], model[0]["full"], model[0]["cand"][5], model[1]["found"]) == (1, 1, slot, 0) and model[0]["n2"] == 4
    old = dict(afr, plane_match=model[0]["match2"][:, :], mp_w=a["mp_w"][0, :5], mp_flags=a["mp_flags"][0, :5], full=a0["full_tab"][0, :0],
               part=a0["part_tab"][0, :0], kf_Rwc=a0["kf_Rwc"][0], kf_coef=list(a0["kf_coef"][0]), kf_npts=list(a0["kf_npts"][0]))
    assert mh.detect_manhattan(old, aprm["mf_ver_th"])[0] == 0               # without the tables the chain writes there is nothing to find
    # ---- the device: one stream for the library and for the tensor operations in between ----
    dev = pcs.dev
    V, P, _, carr = plane_cloud.pack_clouds([S["cf"]] * B, max_planes=pcap)
    _, aarr, _ = plane.pack_associate(frames, pcap, mcap, ptcap)
    tfs = []
    for f in range(B):
        w, h = pmm.pose_layout(model[f]["match2"], a["mp_w"][f, :model[f]["M"]])
        tfs.append(dict(S["fr"], plane_coef=want["plane_coef"], plane_w=w[:, 0:4], par_w=w[:, 4:8], ver_w=w[:, 8:12], plane_has=h & 1,
                        par_has=(h >> 1) & 1, ver_has=(h >> 2) & 1, plane_outlier=np.zeros(K, np.uint8), par_outlier=np.zeros(K, np.uint8),
                        ver_outlier=np.zeros(K, np.uint8)))
    pcaps, parr, pio = pose.pack(tfs, pcap=pcap)
    s = torch.cuda.Stream()
    m = Matcher()
    m.set_stream(s.cuda_stream)
    with torch.cuda.stream(s):
        z = lambda shape, dt, v=0: torch.full(shape, v, dtype=dt, device="cuda")
        i32, f32, u8 = torch.int32, torch.float32, torch.uint8
        d = {k: dev(v.view(np.int32).reshape(B, 4) if k == "frames" else v) for k, v in a0.items()}
        n_out, coef, npts, src = z((B,), i32), z((B, pcap, 4), f32), z((B, pcap), i32), z((B, pcap), i32)
        off, pts, cst = z((B, pcap + 1), i32), z((B, fptcap, 3), f32), z((B, pcap), i32)
        dTcw, dmoff, dmpts = dev(aarr[2]), dev(aarr[5]), dev(aarr[6])
        match, nm, pw, ph = z((B, pcap, 3), i32, -1), z((B,), i32), z((B, pcap, 12), f32), z((B, pcap), u8)
        plane_cloud.plane_clouds_device(m, pcs.prm_record(), B, V, P, pcap, fptcap, [dev(x) for x in carr], n_out, coef, npts, src, off, pts, None, cst)
        plane.plane_association_device(m, plane.plane_params(**aprm), B, (pcap, mcap, ptcap),
                                       [coef, n_out, dTcw, d["mp_w"], d["mp_flags"], dmoff, dmpts, d["n_map"]], match, nm, pw, ph)
        din = dict(frames=dev(keyframe.frame_records(rec).view(np.int32).reshape(B, 10)), depth=z((B, 1), f32), n_cur=z((B,), i32),
                   cur_held=z((B, 1), i32, -1), outlier=z((B, 1), u8), cur_lheld=z((B, 1), i32, -1), line_outlier=z((B, 1), u8),
                   n_cur_lines=z((B,), i32), n_planes=n_out, pt_nobs=z((1,), i32), pt_flags=z((1,), u8), ln_nobs=z((1,), i32),
                   held_id=z((1, 1), i32, -1), n_kps=z((1,), i32), plane_match=match, plane_outlier=z((B, pcap, 3), u8))
        dout = keyframe.keyframe_decision_device(m, keyframe.keyframe_params(**dprm), B, 1, 1, pcap, 1, 1, 1, din,
                                                 keyframe.decision_outputs(B, 1, 1, lambda shape, dt: z(shape, getattr(torch, np.dtype(dt).name))))
        d["frames"][:, 0] = dout["need_kf"]                                   # the gate: the only operation between two library calls
        d.update(plane_coef=coef, plane_npts=npts, n_planes=n_out, Tcw=dTcw, plane_outlier=din["plane_outlier"], plane_match=match)
        tz = lambda shape, dt: z(shape, getattr(torch, np.dtype(dt).name), 0x5A if np.dtype(dt).itemsize == 1 else 0)
        dpo = kfplanes.keyframe_planes_device(m, B, pcap, mcap, kcap, kp.KEYFRAME, d, kfplanes.planes_outputs(B, pcap, tz))
        moff2, mpts2, mst = z((B, mcap + 1), i32), z((B, ptcap, 3), f32), z((B, mcap), i32)
        plane_cloud.map_plane_merge_device(m, pcs.prm_record(), B, (pcap, fptcap, mcap, ptcap),
                                           [n_out, off, pts, None, dpo["merge_into"], dpo["Twc"], dmoff, dmpts, None, d["n_map"]], moff2, mpts2, None, mst)
        d["kf_plane_match"] = dpo["kf_plane_match"]
        doo = kfplanes.manhattan_observe_device(m, plane.plane_params(**aprm), B, pcap, mcap, fcap, qcap, kcap, d, kfplanes.observe_outputs(B, pcap, tz))
        match2, nm2 = z((B, pcap, 3), i32, -1), z((B,), i32)                  # frame t + 1
        plane.plane_association_device(m, plane.plane_params(**aprm), B, (pcap, mcap, ptcap),
                                       [coef, n_out, dTcw, d["mp_w"], d["mp_flags"], moff2, mpts2, d["n_map"]], match2, nm2, pw, ph)
        found, full, choice = z((B,), i32), z((B,), i32), z((B, 6), i32)
        rcw = dev(np.stack([afr["Tcw"].reshape(3, 4)[:, :3].reshape(9)] * B))
        plane.manhattan_detect_device(m, plane.plane_params(**aprm), B, (pcap, mcap, fcap, qcap, kcap),
                                      [coef, npts, n_out, match2, d["mp_flags"], d["n_map"], d["full_tab"], d["n_full"], d["part_tab"], d["n_part"],
                                       d["kf_Rwc"], d["kf_coef"], d["kf_npts"]], found, full, rcw, choice)
        d_parr = [dev(x.view(np.uint8) if x.dtype.names else x) for x in parr]
        d_parr[11], d_parr[12] = pw, ph
        d_io = [dev(x) for x in pio]
        Tout, ng = z((B, 12), f32), z((B,), i32)
        pose.translation_optimization_device(m, pose.pose_params(c), B, pcaps, d_parr, d_io, Tout, ng, rcw=rcw)
    m.sync()
    m.close()
    host = lambda t: t.cpu().numpy()
    assert host(n_out).tolist() == [K] * B and host(coef)[0, :K].tobytes() == want["plane_coef"].tobytes()
    assert host(dout["need_kf"]).tolist() == [1, 0] and host(match)[:, :K].tobytes() == np.stack([x["plane_match"] for x in dec]).tobytes()
    for k in kfplanes.PLANES_INOUT_KEYS + kfplanes.OBSERVE_INOUT_KEYS:
        assert host(d[k]).tobytes() == a[k].tobytes(), k
    for got, exp in ((dpo, po), (doo, oo)):
        for k, v in exp.items():
            g = host(got[k])
            assert all(g[f, :K].tobytes() == v[f, :K].tobytes() for f in range(B)) if v.ndim > 1 and v.shape[1] == pcap else g.tobytes() == v.tobytes(), k
    for f, mo in enumerate(model):
        M, mg = mo["M"], mo["merged"]
        assert np.array_equal(host(moff2)[f, :M + 1], mg["pt_off"]) and np.array_equal(host(mst)[f, :M], mg["status"]), f
        assert host(mpts2)[f, :mg["pt_off"][-1]].tobytes() == np.concatenate(mg["clouds"]).tobytes(), f
        assert int(nm2[f]) == mo["n2"] and np.array_equal(host(match2)[f, :K], mo["match2"]), f
        assert (int(found[f]), int(full[f])) == (mo["found"], mo["full"]), f
        gR = host(rcw)[f]
        if mo["found"]:
            i, j, k3, e, score, kf, _ = mo["cand"]
            assert host(choice)[f].tolist()[:3] == [i, j, k3] and host(choice)[f, 4] == score and host(choice)[f, 5] == kf == slot, f
            assert np.max(np.abs(gR.astype(np.float64) - mo["R"])) <= 2e-6, f
        else:
            assert gR.tobytes() == afr["Tcw"].reshape(3, 4)[:, :3].reshape(9).tobytes(), f
        wn, wT, wout = tm.translation_optimization(tfs[f], c, gR)
        assert int(ng[f]) == wn and wn > 100, f
        assert np.array_equal(host(d_io[0])[f, :len(wout["outlier"])], wout["outlier"]), f
        assert np.array_equal(host(d_io[2])[f, :K, 0], wout["plane_outlier"]), f
        assert np.max(np.abs(host(Tout)[f].astype(np.float64) - wT)) <= 1e-5, f

"""GPU parity: msl_plane_clouds[_batch] and msl_map_plane_merge[_batch] against the sequential model in tests/plane_cloud_model.py.  Every
output must equal the model as bytes, from host memory and from device memory; then one chain on one stream in device memory:
msl_peac_extract_batch -> msl_plane_clouds -> msl_plane_associate -> msl_map_plane_merge -> msl_plane_associate, against the models."""
import numpy as np
import pytest

from tests import plane_cloud_model as pcm
from tests import plane_cloud_scenes as sc

pytestmark = pytest.mark.gpu

F32 = np.float32


_prm, _dev, _clouds_on_device, _as_results = sc.prm_record, sc.dev, sc.clouds_on_device, sc.as_results


def test_scenes_keep_their_margins():
    for fr in (sc.status_frame(), sc.status_frame(11, False), sc.walls_frame(31), sc.walls_frame(32), sc.walls_frame(33, 6, True, 900)):
        assert sc.margins_ok(fr)


@pytest.mark.parametrize("colour", [True, False])
def test_clouds_from_host_memory_equal_the_model(colour):
    from manhattanslam_amd import plane_cloud
    frames = [sc.status_frame(11, colour), sc.walls_frame(31, 4, colour), sc.walls_frame(33, 6, colour, 900)]
    got = plane_cloud.plane_clouds_batch(_prm(), frames, pcap=12, ptcap=6000)
    sc.check_clouds(frames, got, 12, 6000)
    assert [g["n_out"] for g in got] == [5, 4, 6]
    assert got[0]["status"].tolist() == [0, 0, pcm.GATE, pcm.FEW, pcm.FEW, 0, 0, pcm.NO_MODEL, 0, pcm.FEW]


@pytest.mark.parametrize("colour", [True, False])
def test_clouds_from_device_memory_equal_the_model(colour):
    """Device memory, with vertex indices outside the cloud, which are absent there (a host-memory call refuses them)."""
    fr = sc.status_frame(11, colour)
    wild = dict(fr, vertices=[np.concatenate([v[:3], [-5, 10 ** 6, 1 << 17][:3 if i < 2 else 0], v[3:]]).astype(np.int32)
                              for i, v in enumerate(fr["vertices"])])
    frames = [wild, sc.walls_frame(32, 4, colour)]
    sc.check_clouds(frames, _as_results(frames, _clouds_on_device(frames, 10, 5000)), 10, 5000)


def test_a_permutation_of_the_vertices_changes_no_byte():
    from manhattanslam_amd import plane_cloud
    fr = sc.walls_frame(33, 6, True, 900)
    frames = [fr, sc.shuffled(fr, 1), sc.shuffled(fr, 2)]
    got = plane_cloud.plane_clouds_batch(_prm(), frames, pcap=8, ptcap=4000)
    sc.check_clouds(frames[:1], got[:1], 8, 4000)
    for g in got[1:]:
        for k in ("plane_coef", "pts", "rgb", "pt_off", "status", "plane_npts", "plane_src"):
            assert g[k].tobytes() == got[0][k].tobytes(), k


def test_no_room_drops_the_later_planes():
    from manhattanslam_amd import plane_cloud
    frames = [sc.status_frame(11, True)]
    full = pcm.plane_clouds(frames[0], sc.PRM, 64, 1 << 16)
    for pcap, ptcap in ((2, 1 << 12), (10, int(full["pt_off"][2]) + 3)):
        got = plane_cloud.plane_clouds_batch(_prm(), frames, pcap=pcap, ptcap=ptcap)
        sc.check_clouds(frames, got, pcap, ptcap)
        assert got[0]["n_out"] == 2 and (got[0]["status"] == pcm.NO_ROOM).sum() == 3


@pytest.mark.parametrize("colour", [True, False])
def test_merge_from_host_memory_equals_the_model(colour):
    from manhattanslam_amd import plane_cloud
    big = dict(clouds=[sc.block(3, 3, 3), sc.block(1, 1, 1)], merge_into=[0, 0], Twc=sc.IDENTITY,
               mp_clouds=[sc.block(1, 1, 1, (20, 0, 0)), sc.block(2, 1, 1)])
    if colour:
        big.update(rgbs=[np.full((27, 3), 9, np.uint8), np.full((1, 3), 200, np.uint8)], mp_rgbs=[np.full((1, 3), 50, np.uint8), np.full((2, 3), 70, np.uint8)])
    frames = [sc.merge_frame(21, colour), sc.merge_frame(22, colour), big]
    got = plane_cloud.map_plane_merge_batch(_prm(), frames)
    ptcap = max(sum(len(c) for c in fr["mp_clouds"]) for fr in frames)
    sc.check_merge(frames, got, ptcap)                                        # a ptcap the merged map outgrows: NO_ROOM from some row on
    assert got[0]["status"][0] == pcm.MERGED and (got[0]["status"] == pcm.NO_ROOM).any()
    roomy = plane_cloud.map_plane_merge_batch(_prm(), frames, caps=(8, 700, 9, 2000))
    sc.check_merge(frames, roomy, 2000)
    assert roomy[0]["status"].tolist() == [pcm.MERGED, 0, pcm.MERGED, 0, pcm.MERGED, 0]
    assert all(not (g["status"] == pcm.NO_ROOM).any() for g in roomy)


def test_merge_from_device_memory_equals_the_model():
    import torch
    from manhattanslam_amd import plane_cloud
    from manhattanslam_amd.match import Matcher
    frames = [sc.merge_frame(21, True), sc.merge_frame(23, True)]
    caps, arrays = plane_cloud.pack_merge(frames, 7, 600, 8, 1500)
    wild = arrays[4].copy()
    wild[1, 4] = 6                                                            # a row outside [0, n_map): absent on the device, like -1
    arrays[4] = wild
    F, (pcap, fptcap, mcap, ptcap) = len(frames), caps
    d = [_dev(a) for a in arrays]
    off = torch.zeros((F, mcap + 1), dtype=torch.int32, device="cuda")
    pts = torch.zeros((F, ptcap, 3), dtype=torch.float32, device="cuda")
    rgb = torch.zeros((F, ptcap, 3), dtype=torch.uint8, device="cuda")
    st = torch.zeros((F, mcap), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    m = Matcher()
    plane_cloud.map_plane_merge_device(m, _prm(), F, caps, d, off, pts, rgb, st)
    m.sync()
    m.close()
    off, pts, rgb, st = (x.cpu().numpy() for x in (off, pts, rgb, st))
    got = []
    for f, fr in enumerate(frames):
        n = len(fr["mp_clouds"]); o = off[f, :n + 1]
        got.append(dict(clouds=[pts[f, o[j]:o[j + 1]] for j in range(n)], rgbs=[rgb[f, o[j]:o[j + 1]] for j in range(n)], pt_off=o, status=st[f, :n]))
    sc.check_merge(frames, got, ptcap)


def test_host_memory_calls_refuse_bad_indices_with_the_field_named():
    from manhattanslam_amd import MslError, plane_cloud
    fr = sc.walls_frame(31)
    bad = dict(fr, vertices=[np.concatenate([fr["vertices"][0], [len(fr["cloud"]) + 50]]).astype(np.int32)] + fr["vertices"][1:])
    with pytest.raises(MslError, match=r"vertex_indices\[0\]"):
        plane_cloud.plane_clouds_batch(_prm(), [bad], pcap=4, ptcap=4000)
    from manhattanslam_amd._lib import lib, ptr
    V, P, _, arrays = plane_cloud.pack_clouds([fr])
    arrays[2] = arrays[2].copy(); arrays[2][0, 2] = arrays[2][0, 1] - 1       # descending offsets
    outs = [np.zeros(1, np.int32), np.zeros((1, 4, 4), F32), np.zeros((1, 4), np.int32), np.zeros((1, 4), np.int32), np.zeros((1, 5), np.int32),
            np.zeros((1, 4000, 3), F32), None, np.zeros((1, P), np.int32)]
    assert lib.msl_plane_clouds_batch(0, 1, V, P, 4, 4000, ptr(_prm()), *[ptr(a) for a in arrays], 0, *[ptr(a) for a in outs], 0) == -1
    assert b"vertex_offsets" in lib.msl_last_error()
    mf = sc.merge_frame(21, False)
    with pytest.raises(MslError, match=r"merge_into\[0\]\[1\]"):
        plane_cloud.map_plane_merge_batch(_prm(), [dict(mf, merge_into=[0, 6, 4, 0, -1])])
    caps, arrays = plane_cloud.pack_merge([mf])
    for slot, name in ((1, b"pt_off"), (6, b"mp_pt_off")):
        a = [x if x is None else x.copy() for x in arrays]
        a[slot][0, 1] = caps[1 if slot == 1 else 3] + 1
        a[slot][0, 2:] = caps[1 if slot == 1 else 3] + 1
        outs = [np.zeros((1, caps[2] + 1), np.int32), np.zeros((1, caps[3], 3), F32), None, np.zeros((1, caps[2]), np.int32)]
        assert lib.msl_map_plane_merge_batch(0, 1, *caps, ptr(_prm()), *[ptr(x) for x in a], 0, *[ptr(x) for x in outs], 0) == -1
        assert name in lib.msl_last_error(), lib.msl_last_error()
    sc.check_clouds([fr], plane_cloud.plane_clouds_batch(_prm(), [fr], pcap=4, ptcap=4000), 4, 4000)      # the device is still usable


def test_chain_on_one_stream_in_device_memory():
    """msl_peac_extract_batch on a synth frame -> msl_plane_clouds -> msl_plane_associate -> msl_map_plane_merge -> msl_plane_associate of
    the next frame: after the extractor's host outputs are uploaded, nothing returns to the host until the end."""
    import torch
    from manhattanslam_amd import peac, plane, plane_cloud, synth
    from manhattanslam_amd.match import Matcher
    from tests import plane_match_model as pmm
    from tests import plane_scenes
    I = synth.ICL
    _, depth, _, _ = synth.surfel_frame(0, w=640, h=480, intr=I, dropout=0.0)
    d16 = synth.depth_u16(depth)
    P = 16
    _, n, planes, cloud = peac.extract(d16[None], I["fx"], I["fy"], I["cx"], I["cy"], F32(1 / 5000.0), max_planes=P, with_cloud=True)
    rec, vertices = planes[0]
    assert len(rec) >= 1
    fr = dict(cloud=cloud[0], rgb=None, vertices=vertices, planes=[(r["normal"].copy(), r["center"].copy()) for r in rec], seed=77)
    pcap, fptcap, mcap, ptcap = P, P * 512, 8, 4096
    want = pcm.plane_clouds(fr, sc.PRM, pcap, fptcap)
    K = want["n_out"]
    assert K >= 1
    # the map: every kept plane seen from one camera to the left (its cloud moved to the world), then a distractor
    t = np.array([0.05, -0.02, 0.03])
    Twc = np.concatenate([np.eye(3), t[:, None]], axis=1).reshape(12)
    Tcw = np.concatenate([np.eye(3), -t[:, None]], axis=1).reshape(12).astype(F32)
    clouds = [want["pts"][want["pt_off"][k]:want["pt_off"][k + 1]] for k in range(K)]
    rows = min(K, mcap - 1)
    mp_clouds = [pcm.voxel_grid(pcm.transform(Twc, clouds[k])[::2], None, 0.2)[1] for k in range(rows)] + [sc.block(2, 2, 1, (40, 40, 40))]
    mp_w = np.array([np.append(want["plane_coef"][k, :3], want["plane_coef"][k, 3] - want["plane_coef"][k, :3].astype(np.float64) @ t) for k in range(rows)] +
                    [[0.0, 0.0, 1.0, -8.1]], F32)
    aprm = plane_scenes.params()
    afr = dict(plane_coef=want["plane_coef"], Tcw=Tcw, plane_match=np.full((K, 3), -1, np.int32), mp_w=mp_w, mp_flags=np.ones(len(mp_w), np.uint8),
               mp_clouds=mp_clouds)
    n1, match1, _ = pmm.search_map_by_coefficients(afr, aprm)
    assert n1 >= 1
    mfr = dict(clouds=clouds, rgbs=None, merge_into=[int(x) for x in match1[:, 0]], Twc=Twc, mp_clouds=mp_clouds, mp_rgbs=None)
    merged = pcm.map_plane_merge(mfr, sc.PRM, ptcap)
    n2, match2, _ = pmm.search_map_by_coefficients(dict(afr, plane_match=match1, mp_clouds=merged["clouds"]), aprm)
    # the device: one stream for the library and for the one tensor operation in between
    V, _, _, arrays = plane_cloud.pack_clouds([fr], max_planes=P)
    s = torch.cuda.Stream()
    m = Matcher()
    m.set_stream(s.cuda_stream)
    with torch.cuda.stream(s):
        d = [_dev(a) for a in arrays]
        z = lambda shape, dt, v=0: torch.full(shape, v, dtype=dt, device="cuda")
        n_out, coef, npts, src = z((1,), torch.int32), z((1, pcap, 4), torch.float32), z((1, pcap), torch.int32), z((1, pcap), torch.int32)
        off, pts, status = z((1, pcap + 1), torch.int32), z((1, fptcap, 3), torch.float32), z((1, P), torch.int32)
        _, a_in, _ = plane.pack_associate([afr], pcap, mcap, ptcap)
        dTcw, dw, dflags, dmoff, dmpts, dnmap = (_dev(a) for a in a_in[2:])
        match = z((1, pcap, 3), torch.int32, -1)
        nm, pw, ph = z((1,), torch.int32), z((1, pcap, 12), torch.float32), z((1, pcap), torch.uint8)
        moff2, mpts2, mst = z((1, mcap + 1), torch.int32), z((1, ptcap, 3), torch.float32), z((1, mcap), torch.int32)
        nm2 = z((1,), torch.int32)
        dTwc = _dev(Twc[None])
        plane_cloud.plane_clouds_device(m, _prm(), 1, V, P, pcap, fptcap, d, n_out, coef, npts, src, off, pts, None, status)
        plane.plane_association_device(m, plane.plane_params(**aprm), 1, (pcap, mcap, ptcap), [coef, n_out, dTcw, dw, dflags, dmoff, dmpts, dnmap],
                                       match, nm, pw, ph)
        into = match[:, :, 0].contiguous()
        plane_cloud.map_plane_merge_device(m, _prm(), 1, (pcap, fptcap, mcap, ptcap), [n_out, off, pts, None, into, dTwc, dmoff, dmpts, None, dnmap],
                                           moff2, mpts2, None, mst)
        plane.plane_association_device(m, plane.plane_params(**aprm), 1, (pcap, mcap, ptcap), [coef, n_out, dTcw, dw, dflags, moff2, mpts2, dnmap],
                                       match, nm2, pw, ph)
    m.sync()
    m.close()
    assert int(n_out[0]) == K and coef[0, :K].cpu().numpy().tobytes() == want["plane_coef"].tobytes()
    assert np.array_equal(status[0, :len(rec)].cpu().numpy(), want["status"])
    assert int(nm[0]) == n1 and int(nm2[0]) == n2 and np.array_equal(match[0, :K].cpu().numpy(), match2)
    assert np.array_equal(into[0, :K].cpu().numpy(), match1[:, 0])
    M = len(mp_clouds)
    assert np.array_equal(moff2[0, :M + 1].cpu().numpy(), merged["pt_off"]) and np.array_equal(mst[0, :M].cpu().numpy(), merged["status"])
    assert mpts2[0, :merged["pt_off"][-1]].cpu().numpy().tobytes() == np.concatenate(merged["clouds"]).tobytes()
    assert (merged["status"] == pcm.MERGED).sum() >= 1

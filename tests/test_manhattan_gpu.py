"""GPU parity: batched Manhattan-frame detection (msl_manhattan_detect[_batch], Tracking::DetectManhattan) vs the sequential CPU model in
tests/manhattan_model.py: found, full and choice identical, Rcw within 2e-6 (the polar factor is computed differently, see include/msl.h)
and untouched where nothing is found.  Last, the device chain of the Manhattan branch on one handle: plane association -> detection ->
translation-only optimisation, every intermediate in device memory."""
import numpy as np
import pytest

from manhattanslam_amd import plane
from tests import manhattan_model as mm
from tests import plane_match_model as pmm
from tests import plane_scenes as sc

pytestmark = pytest.mark.gpu

PRM = sc.params()
RTOL = 2e-6


def _prm():
    return plane.plane_params(**PRM)


def _associated(fr):
    return dict(fr, plane_match=pmm.search_map_by_coefficients(fr, PRM)[1])


def _ragged():
    specs = [dict(seed=4001 + s, n_frame=int(4 + s % 9)) for s in range(10)] + \
        [dict(seed=4020, n_frame=0), dict(seed=4021, n_frame=1), dict(seed=4022, n_walls=6, n_distract=30, n_frame=30, pts=(1, 4)),
         dict(seed=4023, n_kf=1, bad=0.6)]
    return [_associated(sc.room(**s)[0]) for s in specs]


def _check(frames, got, rcw_in):
    nfound = nfull = 0
    for f, fr in enumerate(frames):
        found, full, R, cand = mm.detect_manhattan(fr, PRM["mf_ver_th"], rcw_in[f])
        gf, gfull, gR, gch = got[f]
        assert (gf, gfull) == (found, full), (f, gf, gfull, found, full)
        if not found:
            assert gR.tobytes() == rcw_in[f].tobytes() and gch.tolist() == [-1, -1, -1, -1, 0, -1], f
            continue
        nfound += 1; nfull += full
        i, j, k, e, score, kf, _ = cand
        norm = plane.sort_full if k >= 0 else plane.sort_part
        tab = norm(fr["full"] if k >= 0 else fr["part"])
        assert gch.tolist()[:3] == [i, j, k] and gch[4] == score and gch[5] == kf, (f, gch, cand[:6])
        assert np.array_equal(tab[gch[3]], norm([e])[0]), f                  # the same entry of the sorted table
        assert np.max(np.abs(gR.astype(np.float64) - R)) <= RTOL, (f, gR, R)
    return nfound, nfull


def test_ragged_batch_matches_model():
    frames = _ragged()
    rcw_in = np.random.default_rng(1).normal(size=(len(frames), 9)).astype(np.float32)
    got = plane.manhattan_detect_batch(_prm(), frames, rcw_in)
    nfound, nfull = _check(frames, got, rcw_in)
    assert nfound >= 6 and 0 < nfull < nfound


def test_deterministic_independent_of_the_batch_and_of_the_memory_kind():
    import torch
    from manhattanslam_amd.match import Matcher
    frames = _ragged()
    F = len(frames)
    rcw_in = np.zeros((F, 9), np.float32)
    caps = (48, 80, 64, 64, 8)
    a = plane.manhattan_detect_batch(_prm(), frames, rcw_in, caps=caps)
    m = Matcher()
    b = plane.manhattan_detect_batch(_prm(), frames, rcw_in, handle=m, caps=caps)
    parts = plane.manhattan_detect_batch(_prm(), frames[:5], rcw_in[:5], handle=m, caps=caps) + \
        plane.manhattan_detect_batch(_prm(), frames[5:], rcw_in[5:], handle=m, caps=caps)
    for x, y, z in zip(a, b, parts):
        for u, v, w in zip(x, y, z):
            assert np.asarray(u).tobytes() == np.asarray(v).tobytes() == np.asarray(w).tobytes()
    caps2, arrays = plane.pack_manhattan(frames, *caps)
    d = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in arrays]
    found = torch.full((F,), -3, dtype=torch.int32, device="cuda")
    full = torch.full((F,), -3, dtype=torch.int32, device="cuda")
    R = torch.zeros((F, 9), dtype=torch.float32, device="cuda")
    ch = torch.zeros((F, 6), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    plane.manhattan_detect_device(m, _prm(), F, caps2, d, found, full, R, ch)
    m.sync()
    m.close()
    for f in range(F):
        assert (int(found[f]), int(full[f])) == a[f][:2]
        assert R[f].cpu().numpy().tobytes() == a[f][2].tobytes() and ch[f].cpu().numpy().tobytes() == a[f][3].tobytes()
    _check(frames, a, rcw_in)


@pytest.mark.parametrize("what", ["pcap", "mcap", "fcap", "qcap", "kcap", "unsorted_full", "unsorted_part"])
def test_limits_and_unsorted_tables_are_refused_without_a_launch(what):
    from manhattanslam_amd import MslError
    from manhattanslam_amd._lib import check, lib, ptr
    fr = _associated(sc.room(4050, n_frame=8)[0])
    caps = dict(pcap=16, mcap=16, fcap=8, qcap=12, kcap=4)
    (pc, mc, fc, qc, kc), arrays = plane.pack_manhattan([fr], *caps.values())
    if what.startswith("unsorted"):
        t = arrays[6] if what == "unsorted_full" else arrays[8]
        n = arrays[7] if what == "unsorted_full" else arrays[9]
        w = 3 if what == "unsorted_full" else 2
        n[0] = max(n[0], 2)
        t[0, 0, :w], t[0, 1, :w] = list(range(5, 5 + w)), list(range(w))  # two entries out of order
        big = (pc, mc, fc, qc, kc)
        named = r"%s\[0\] is not sorted by its keys at entry 1" % ("full_tab" if what == "unsorted_full" else "part_tab")
    else:
        over = dict(pcap=65, mcap=4097, fcap=65537, qcap=65537, kcap=4097)
        big = tuple(over[k] if k == what else v for k, v in caps.items())
        named = r"%s %d outside 1 \.\. %d" % (what, over[what], over[what] - 1)
    out = [np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros((1, 9), np.float32), None]
    with pytest.raises(MslError, match=r"\(-1\): msl_manhattan_detect: " + named + "$"):   # refused before the arrays are read on the device
        check(lib.msl_manhattan_detect_batch(0, 1, *big, ptr(_prm()), *[ptr(a) for a in arrays], 0, *[ptr(a) for a in out], 0),
              "msl_manhattan_detect_batch")
    r0 = np.zeros((1, 9), np.float32)
    _check([fr], plane.manhattan_detect_batch(_prm(), [fr], r0), r0)          # the device is still usable


def test_device_chain_of_the_manhattan_branch():
    """Tracking::Track's Manhattan branch on one handle, device memory throughout: msl_plane_associate (plane_w / plane_has in the pose
    layout) -> msl_manhattan_detect (Rcw) -> msl_pose_optimize_translation reading both.  found, the plane bytes, n_good and every
    outlier flag equal the CPU models fed the same arrays; Tcw_out within 1e-5."""
    import torch
    from manhattanslam_amd import pose
    from manhattanslam_amd.match import Matcher
    from tests import pose_scenes as ps
    from tests import translation_model as tm
    from tests import translation_scenes as ts
    c = ps.params()
    rows, seed = [], 6000
    while len(rows) < 4:                                                      # scenes whose translation margins pass
        seed += 1
        fr, Rt, tt = ps.scene(seed, n_pts=600, n_lines=8, n_planes=0, margin=None, c=c)
        room = _associated(sc.room(seed, n_frame=6, noise_deg=0.2, pose=(Rt, tt), empty=False, nan=False, bad=0.0, init_match=0.0)[0])
        room["Tcw"] = fr["Tcw"]                                               # the frame's (perturbed) pose, as the tracker has it
        n, match, _ = pmm.search_map_by_coefficients(dict(room, plane_match=np.full((len(room["plane_coef"]), 3), -1, np.int32)), PRM)
        found, _, R, _ = mm.detect_manhattan(dict(room, plane_match=match), PRM["mf_ver_th"])
        if not found or n < 3:
            continue
        w, h = pmm.pose_layout(match, room["mp_w"])
        K = len(room["plane_coef"])
        tf = dict(fr, plane_coef=room["plane_coef"], plane_w=w[:, 0:4], par_w=w[:, 4:8], ver_w=w[:, 8:12], plane_has=h & 1,
                  par_has=(h >> 1) & 1, ver_has=(h >> 2) & 1, plane_outlier=np.zeros(K, np.uint8), par_outlier=np.zeros(K, np.uint8),
                  ver_outlier=np.zeros(K, np.uint8))
        try:
            ts.check_margin(tf, c, R)
        except AssertionError:
            continue
        room["plane_match"] = np.full((K, 3), -1, np.int32)
        rows.append((tf, room, match, w, h, R))
    tfs, rooms = [r[0] for r in rows], [r[1] for r in rows]
    B = len(rows)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a.view(np.uint8) if a.dtype.names else a)).cuda()   # keypoints as bytes
    pcap = max(max(len(r["plane_coef"]), max(len(k) for k in r["kf_coef"])) for r in rooms)   # keyframe planes share the cap
    acaps, aarr, amatch = plane.pack_associate(rooms, pcap=pcap)
    mcaps, marr = plane.pack_manhattan(rooms, pcap=acaps[0], mcap=acaps[1])
    pcaps, parr, pio = pose.pack(tfs, pcap=pcap)
    d_match = dev(amatch)
    nm = torch.zeros(B, dtype=torch.int32, device="cuda")
    pw = torch.zeros((B, pcap, 12), dtype=torch.float32, device="cuda")
    ph = torch.zeros((B, pcap), dtype=torch.uint8, device="cuda")
    d_marr = [dev(a) for a in marr]
    d_marr[3] = d_match                                                       # detection reads the association's plane_match
    found = torch.zeros(B, dtype=torch.int32, device="cuda")
    full = torch.zeros(B, dtype=torch.int32, device="cuda")
    rcw = torch.zeros((B, 9), dtype=torch.float32, device="cuda")
    d_parr = [dev(a) for a in parr]
    d_parr[11], d_parr[12] = pw, ph                                           # the optimiser reads plane_w / plane_has in place
    d_io = [dev(a) for a in pio]
    Tout = torch.zeros((B, 12), dtype=torch.float32, device="cuda")
    ng = torch.zeros(B, dtype=torch.int32, device="cuda")
    d_aarr = [dev(a) for a in aarr]
    torch.cuda.synchronize()
    m = Matcher()
    plane.plane_association_device(m, _prm(), B, acaps, d_aarr, d_match, nm, pw, ph)
    plane.manhattan_detect_device(m, _prm(), B, mcaps, d_marr, found, full, rcw)
    pose.translation_optimization_device(m, pose.pose_params(c), B, pcaps, d_parr, d_io, Tout, ng, rcw=rcw)
    m.sync()
    m.close()
    for f, (tf, room, match, w, h, R) in enumerate(rows):
        K = len(room["plane_coef"])
        assert int(found[f]) == 1 and np.array_equal(d_match[f, :K].cpu().numpy(), match), f
        assert pw[f, :K].cpu().numpy().tobytes() == w.tobytes() and np.array_equal(ph[f, :K].cpu().numpy(), h), f
        assert np.max(np.abs(rcw[f].cpu().numpy().astype(np.float64) - R)) <= RTOL, f
        wn, wT, wout = tm.translation_optimization(tf, c, rcw[f].cpu().numpy())
        assert int(ng[f]) == wn and wn > 100, f
        n, nl = len(tf["pt_ref"]), len(tf["line_has"])
        assert np.array_equal(d_io[0][f, :n].cpu().numpy(), wout["outlier"]), f
        assert np.array_equal(d_io[1][f, :nl].cpu().numpy(), wout["line_outlier"]), f
        assert np.array_equal(d_io[2][f, :K, 0].cpu().numpy(), wout["plane_outlier"]), f
        assert np.max(np.abs(Tout[f].cpu().numpy().astype(np.float64) - wT)) <= 1e-5, f

"""msl_plane_clouds and msl_map_plane_merge at the limits include/msl.h states: a cloud of exactly MSL_PLANE_CLOUD_MAX_VOXELS voxels and one
above, pcap / mcap / ptcap / n_vertices at their limits and refused above them, clamped counts, device-memory rows beyond the counts, and
the grid overflow.  Every result is the sequential model's (tests/plane_cloud_model.py), as bytes."""
import numpy as np
import pytest

from tests import plane_cloud_model as pcm
from tests import plane_cloud_scenes as sc

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
_prm = sc.prm_record


def _flat(nx, ny, z=2.1):
    """One vertex at the centre of every cell of an nx x ny sheet of the plane z = const: nx * ny voxels, an exact plane."""
    p = sc.block(nx, ny, 1).astype(F64)
    p[:, 2] = z
    return p


def _frame(sheets, seed=5):
    fr = sc.Frame(seed, False)
    for p in sheets:
        fr.add(p, (0, 0, 1), (0.1, 0.1, p[0, 2] if len(p) else 1.0))
    return fr.done()


def test_voxel_limit_exactly_and_one_above():
    from manhattanslam_amd import plane_cloud
    over = np.concatenate([_flat(64, 64), [[64 * 0.2 + 0.1, 0.1, 2.1]]])
    frames = [_frame([_flat(64, 64), over, _flat(3, 3)])]
    assert sc.margins_ok(frames[0])
    got = plane_cloud.plane_clouds_batch(_prm(), frames, pcap=3, ptcap=5000)
    sc.check_clouds(frames, got, 3, 5000)
    assert got[0]["status"].tolist() == [pcm.KEPT, pcm.VOXELS, pcm.KEPT] and got[0]["plane_npts"].tolist() == [4096, 9]
    # the merge: 4095 voxels + one new is merged; 4096 + one new is refused and the row keeps its cloud
    sheet = _flat(64, 64).astype(F32)
    extra = np.array([[64 * 0.2 + 0.1, 0.1, 2.1]], F32)
    fr = dict(clouds=[extra, extra], rgbs=None, merge_into=[0, 1], Twc=sc.IDENTITY, mp_clouds=[sheet[:4095], sheet, sheet[:5]], mp_rgbs=None)
    res = plane_cloud.map_plane_merge_batch(_prm(), [fr], caps=(2, 2, 3, 9000))
    sc.check_merge([fr], res, 9000)
    assert res[0]["status"].tolist() == [pcm.MERGED, pcm.VOXELS, 0] and [len(c) for c in res[0]["clouds"]] == [4096, 4096, 5]


def test_accumulators_in_lds_and_in_the_slab():
    """Clouds of 1024 voxels (the last that accumulates in LDS) and of 1025 (the first that takes the global slab), three vertices and three
    colours per voxel, through both entry points."""
    from manhattanslam_amd import plane_cloud
    rng = np.random.default_rng(14)
    grid = [(ix, iy) for iy in range(32) for ix in range(32)]
    fr = sc.Frame(6, True)
    for cells in (grid, grid + [(32, 0)], grid[:1023]):
        fr.add(sc.cells(rng, cells, 2.13, per_cell=3), (0, 0, 1), (0.1, 0.1, 2.13))
    frames = [fr.done()]
    assert sc.margins_ok(frames[0])
    got = plane_cloud.plane_clouds_batch(_prm(), frames, pcap=3, ptcap=4000)
    sc.check_clouds(frames, got, 3, 4000)
    assert got[0]["plane_npts"].tolist() == [1024, 1025, 1023]
    col = lambda c: rng.integers(0, 256, (len(c), 3)).astype(np.uint8)
    one = sc.cells(rng, [(32, 0)], 2.13, per_cell=2).astype(F32)
    two = sc.cells(rng, [(32, 0), (32, 1)], 2.13, per_cell=2).astype(F32)
    row = sc.cells(rng, grid[:1023], 2.13, per_cell=3).astype(F32)
    mf = dict(clouds=[one, two], merge_into=[0, 1], Twc=sc.IDENTITY, mp_clouds=[row, row], rgbs=[col(one), col(two)], mp_rgbs=[col(row), col(row)])
    res = plane_cloud.map_plane_merge_batch(_prm(), [mf], caps=(2, 8, 2, 7000))
    sc.check_merge([mf], res, 7000)
    assert [len(c) for c in res[0]["clouds"]] == [1024, 1025] and res[0]["status"].tolist() == [pcm.MERGED, pcm.MERGED]


def test_grid_overflow():
    from manhattanslam_amd import plane_cloud
    far = np.array([[-30000.0, -30000.0, -30000.0], [30000.0, 30000.0, 30000.0], [0.1, 0.1, 0.1]])
    frames = [_frame([far, _flat(3, 3)])]
    got = plane_cloud.plane_clouds_batch(_prm(), frames, pcap=2, ptcap=100)
    sc.check_clouds(frames, got, 2, 100)
    assert got[0]["status"].tolist() == [pcm.GRID, pcm.KEPT]
    fr = dict(clouds=[far[1:2].astype(F32), sc.block(1, 1, 1)], rgbs=None, merge_into=[0, 1], Twc=sc.IDENTITY,
              mp_clouds=[far[:1].astype(F32), sc.block(2, 1, 1)], mp_rgbs=None)
    res = plane_cloud.map_plane_merge_batch(_prm(), [fr], caps=(2, 4, 2, 16))
    sc.check_merge([fr], res, 16)
    assert res[0]["status"].tolist() == [pcm.GRID, pcm.MERGED] and res[0]["clouds"][0].tobytes() == far[:1].astype(F32).tobytes()


def test_pcap_and_max_planes_at_64():
    from manhattanslam_amd import plane_cloud
    rng = np.random.default_rng(9)
    sheets = [sc.cells(rng, [(0, 0), (3, 0), (0, 3), (3, 4), (5, 1)][:4 + i % 2], 1.13 + 0.3 * (i % 7), per_cell=2) for i in range(64)]
    frames = [_frame(sheets)]
    assert sc.margins_ok(frames[0])
    got = plane_cloud.plane_clouds_batch(_prm(), frames, pcap=64, ptcap=400)
    sc.check_clouds(frames, got, 64, 400)
    assert got[0]["n_out"] == 64 and got[0]["plane_src"].tolist() == list(range(64))


def test_n_vertices_and_ptcap_at_their_limits():
    """2^17 vertices in one plane; ptcap = 2^22 with the last point of the array written."""
    from manhattanslam_amd import plane_cloud
    rng = np.random.default_rng(10)
    V = 1 << 17
    p = np.concatenate([rng.uniform(0, 6.0, (V, 2)), np.full((V, 1), 2.1)], axis=1)
    fr = dict(cloud=p, rgb=None, vertices=[np.arange(V, dtype=np.int32)], planes=[(np.array([0.0, 0, 1]), np.array([1.0, 1, 2.1]))], seed=3)
    assert sc.margins_ok(fr)
    got = plane_cloud.plane_clouds_batch(_prm(), [fr], pcap=1, ptcap=1 << 22)
    sc.check_clouds([fr], got, 1, 1 << 22)
    assert got[0]["plane_npts"].tolist() == [900]
    # the merge with ptcap = 2^22: the map's last row ends at the last point of the array and is merged in place of itself
    from manhattanslam_amd._lib import lib, ptr
    cap = 1 << 22
    mp_off = np.array([[0, cap - 3, cap]], np.int32)
    mp_pts = np.zeros((1, cap, 3), F32)
    tail = sc.block(3, 1, 1)
    mp_pts[0, cap - 3:] = tail
    mp_pts[0, :cap - 3] = sc.block(1, 1, 1, (7, 7, 7))[0]
    inputs = [np.array([1], np.int32), np.array([[0, 1]], np.int32), sc.block(1, 1, 1, (3, 0, 0)).reshape(1, 1, 3), None, np.array([[1]], np.int32),
              sc.IDENTITY.reshape(1, 12), mp_off, mp_pts, None, np.array([2], np.int32)]
    off = np.zeros((1, 3), np.int32); out = np.zeros((1, cap, 3), F32); st = np.zeros((1, 2), np.int32)
    assert lib.msl_map_plane_merge_batch(0, 1, 1, 1, 2, cap, ptr(_prm()), *[ptr(a) for a in inputs], 0, ptr(off), ptr(out), None, ptr(st), 0) == 0
    assert off.tolist() == [[0, cap - 3, cap - 3]] and st.tolist() == [[0, pcm.NO_ROOM]]       # 4 merged points do not fit behind cap - 3
    assert out[0, :cap - 3].tobytes() == mp_pts[0, :cap - 3].tobytes()
    inputs[4] = np.array([[-1]], np.int32)
    assert lib.msl_map_plane_merge_batch(0, 1, 1, 1, 2, cap, ptr(_prm()), *[ptr(a) for a in inputs], 0, ptr(off), ptr(out), None, ptr(st), 0) == 0
    assert off.tolist() == [[0, cap - 3, cap]] and st.tolist() == [[0, 0]] and out.tobytes() == mp_pts.tobytes()


def test_mcap_at_4096():
    from manhattanslam_amd import plane_cloud
    rng = np.random.default_rng(12)
    mp = [np.zeros((0, 3), F32)] * 4096
    for j in (0, 1, 2047, 4094, 4095):
        mp[j] = sc.wall(rng, (0, 0, 1), (j * 0.001, 0, 2.1), (0.5, 0.5), 20).astype(F32)
    fr = dict(clouds=[sc.block(2, 2, 1), sc.block(1, 2, 1), sc.block(2, 1, 1)], rgbs=None, merge_into=[4095, 2047, 4095], Twc=sc.pose(4), mp_clouds=mp,
              mp_rgbs=None)
    res = plane_cloud.map_plane_merge_batch(_prm(), [fr], caps=(3, 16, 4096, 256))
    sc.check_merge([fr], res, 256)
    st = res[0]["status"]
    assert st[4095] == pcm.MERGED and st[2047] == pcm.MERGED and st.sum() == 2


@pytest.mark.parametrize("what", ["pcap", "max_planes", "n_vertices", "ptcap", "mcap", "merge_ptcap", "fptcap", "leaf", "max_iterations", "probability",
                                  "colour"])
def test_limits_are_refused_without_a_launch(what):
    from manhattanslam_amd import plane_cloud
    from manhattanslam_amd._lib import lib, ptr
    fr = _frame([_flat(3, 3)])
    V, P, _, arrays = plane_cloud.pack_clouds([fr])
    caps = dict(n_vertices=V, max_planes=P, pcap=4, ptcap=64)
    prm = _prm()
    one = np.zeros(8, np.int32)                                               # small arrays: the refusal comes before any staging
    outs = [one, np.zeros(16, F32), one, one, one, np.zeros(192, F32), None, one]
    mcaps = dict(pcap=1, fptcap=4, mcap=2, ptcap=16)
    minputs = [np.array([1], np.int32), np.array([[0, 1]], np.int32), np.zeros((1, 4, 3), F32), None, np.array([[0]], np.int32), sc.IDENTITY.reshape(1, 12),
               np.zeros((1, 3), np.int32), np.zeros((1, 16, 3), F32), None, np.array([2], np.int32)]
    mouts = [np.zeros((1, 3), np.int32), np.zeros((1, 16, 3), F32), None, np.zeros((1, 2), np.int32)]
    merge = what in ("mcap", "merge_ptcap", "fptcap")
    if what in ("pcap", "max_planes"):
        caps[what] = 65
    elif what == "n_vertices":
        caps[what] = (1 << 17) + 1
    elif what == "ptcap":
        caps[what] = (1 << 22) + 1
    elif what == "mcap":
        mcaps["mcap"] = 4097
    elif what == "merge_ptcap":
        mcaps["ptcap"] = (1 << 22) + 1
    elif what == "fptcap":
        mcaps["fptcap"] = (1 << 22) + 1
    elif what == "leaf":
        prm["leaf"] = 0.03
    elif what == "max_iterations":
        prm["max_iterations"] = 0
    elif what == "probability":
        prm["probability"] = 1.5
    elif what == "colour":
        outs[6] = np.zeros(192, np.uint8)                                     # rgb_out without rgb
    if merge:
        rc = lib.msl_map_plane_merge_batch(0, 1, mcaps["pcap"], mcaps["fptcap"], mcaps["mcap"], mcaps["ptcap"], ptr(prm), *[ptr(a) for a in minputs], 0,
                                           *[ptr(a) for a in mouts], 0)
    else:
        rc = lib.msl_plane_clouds_batch(0, 1, caps["n_vertices"], caps["max_planes"], caps["pcap"], caps["ptcap"], ptr(prm), *[ptr(a) for a in arrays], 0,
                                        *[ptr(a) for a in outs], 0)
    assert rc == -1 and lib.msl_last_error()
    got = plane_cloud.plane_clouds_batch(_prm(), [fr], pcap=4, ptcap=64)      # the device is still usable
    sc.check_clouds([fr], got, 4, 64)


def test_counts_are_clamped():
    from manhattanslam_amd import plane_cloud
    from manhattanslam_amd._lib import lib, ptr
    fr = sc.walls_frame(31)
    V, P, _, arrays = plane_cloud.pack_clouds([fr, fr])
    arrays[5] = np.array([1000, -3], np.int32)                                # n_planes: all of max_planes, and none
    pcap, ptcap = 6, 3000
    outs = [np.zeros(2, np.int32), np.zeros((2, pcap, 4), F32), np.zeros((2, pcap), np.int32), np.zeros((2, pcap), np.int32),
            np.zeros((2, pcap + 1), np.int32), np.zeros((2, ptcap, 3), F32), None, np.full((2, P), -9, np.int32)]
    assert lib.msl_plane_clouds_batch(0, 2, V, P, pcap, ptcap, ptr(_prm()), *[ptr(a) for a in arrays], 0, *[ptr(a) for a in outs], 0) == 0
    res = sc.as_results([fr, dict(fr, planes=[], vertices=[])], outs)
    sc.check_clouds([fr], res[:1], pcap, ptcap)
    assert res[1]["n_out"] == 0 and outs[7][1].tolist() == [-9] * P and outs[4][1, 0] == 0
    mf = sc.merge_frame(21, False)
    caps, marr = plane_cloud.pack_merge([mf, mf], 5, 400, 6, 1000)
    marr[0] = np.array([99, 0], np.int32)                                     # n_planes beyond pcap, and none
    marr[9] = np.array([77, -1], np.int32)                                    # n_map beyond mcap, and an empty map
    off = np.zeros((2, 7), np.int32); pts = np.zeros((2, 1000, 3), F32); st = np.full((2, 6), -9, np.int32)
    assert lib.msl_map_plane_merge_batch(0, 2, *caps, ptr(_prm()), *[ptr(a) for a in marr], 0, ptr(off), ptr(pts), None, ptr(st), 0) == 0
    want = pcm.map_plane_merge(mf, sc.PRM, 1000)
    assert np.array_equal(off[0], want["pt_off"]) and np.array_equal(st[0], want["status"])
    assert pts[0, :off[0, -1]].tobytes() == np.concatenate(want["clouds"]).tobytes()
    assert off[1, 0] == 0 and st[1].tolist() == [-9] * 6


def test_device_memory_rows_beyond_the_counts_keep_their_bytes():
    import torch
    from manhattanslam_amd import plane_cloud
    from manhattanslam_amd.match import Matcher
    frames = [sc.walls_frame(31), sc.status_frame(11, False)]                 # 4 and 10 detector planes: max_planes is 10
    pcap, ptcap = 12, 3000
    raw = sc.clouds_on_device(frames, pcap, ptcap, fill=77)
    sc.check_clouds(frames, sc.as_results(frames, raw), pcap, ptcap)
    n_out, coef, npts, src, off, pts, _, status = raw
    for f in range(2):
        n = int(n_out[f])
        assert n < pcap and (coef[f, n:] == 77).all() and (npts[f, n:] == 77).all() and (src[f, n:] == 77).all() and (off[f, n + 1:] == 77).all()
        assert (pts[f, off[f, n]:] == 77).all()
    assert (status[0, 4:] == 77).all()
    mfs = [sc.merge_frame(21, False), dict(sc.merge_frame(22, False))]
    mfs[1]["mp_clouds"] = mfs[1]["mp_clouds"][:5]                             # five rows: its plane 4 stays -1, nothing names row 5
    caps, arrays = plane_cloud.pack_merge(mfs, 6, 500, 9, 1200)
    d = [sc.dev(a) for a in arrays]
    off = torch.full((2, 10), 77, dtype=torch.int32, device="cuda")
    out = torch.full((2, 1200, 3), 77.0, dtype=torch.float32, device="cuda")
    st = torch.full((2, 9), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    m = Matcher()
    plane_cloud.map_plane_merge_device(m, _prm(), 2, caps, d, off, out, None, st)
    m.sync()
    m.close()
    off, out, st = off.cpu().numpy(), out.cpu().numpy(), st.cpu().numpy()
    for f, fr in enumerate(mfs):
        n = len(fr["mp_clouds"])
        want = pcm.map_plane_merge(fr, sc.PRM, 1200)
        assert np.array_equal(off[f, :n + 1], want["pt_off"]) and np.array_equal(st[f, :n], want["status"])
        assert out[f, :off[f, n]].tobytes() == np.concatenate(want["clouds"]).tobytes()
        assert (off[f, n + 1:] == 77).all() and (st[f, n:] == 77).all() and (out[f, off[f, n]:] == 77).all()

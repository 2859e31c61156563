"""GPU parity: batched plane association (msl_plane_associate[_batch], PlaneMatcher::SearchMapByCoefficients) vs the sequential CPU model
in tests/plane_match_model.py.  plane_match, nmatches, plane_w, plane_has and pM must be bit-identical, with the in/out plane_match carried
from a first call into a second one."""
import numpy as np
import pytest

from tests import plane_match_model as pmm
from tests import plane_scenes as sc

pytestmark = pytest.mark.gpu

PRM = sc.params()


def _prm():
    from manhattanslam_amd import plane
    return plane.plane_params(**PRM)


def _ragged():
    specs = [dict(seed=3001), dict(seed=3002, n_frame=0), dict(seed=3003, n_walls=3, n_distract=0), dict(seed=3004, pts=(0, 0)),
             dict(seed=3005, pts=(300, 900), n_distract=20), dict(seed=3006, bad=0.5), dict(seed=3007, n_frame=14, n_distract=40),
             dict(seed=3008, pts=(1, 3)), dict(seed=3009, init_match=1.0), dict(seed=3010, n_walls=6, n_distract=58, n_frame=40)]
    frames = [sc.room(**s)[0] for s in specs]
    nomap = sc.room(3011)[0]                                                  # a frame with no map planes
    nomap.update(mp_w=np.zeros((0, 4), np.float32), mp_flags=np.zeros(0, np.uint8), mp_clouds=[])
    return frames + [nomap]


def _check(frames, got):
    for f, fr in enumerate(frames):
        n, match, pM = pmm.search_map_by_coefficients(fr, PRM)
        w, h = pmm.pose_layout(match, fr["mp_w"])
        g = got[f]
        assert g["nmatches"] == n, f
        assert np.array_equal(g["plane_match"], match), (f, g["plane_match"], match)
        assert g["plane_w"].tobytes() == w.tobytes() and np.array_equal(g["plane_has"], h), f
        assert g["pM"].tobytes() == pM.tobytes(), f


def test_ragged_batch_matches_model_and_carries_state():
    from manhattanslam_amd import plane
    frames = _ragged()
    a = plane.plane_association_batch(_prm(), frames)
    _check(frames, a)
    assert sum(x["nmatches"] for x in a) > 20
    rng = np.random.default_rng(5)
    second = []
    for fr, x in zip(frames, a):                                              # the next frame: moved a little, the matches carried
        T = fr["Tcw"].copy()
        T[[3, 7, 11]] += rng.normal(size=3).astype(np.float32) * 0.3
        second.append(dict(fr, Tcw=T, plane_match=x["plane_match"]))
    b = plane.plane_association_batch(_prm(), second)
    _check(second, b)
    kept = sum(int(np.sum((x["plane_match"][:, 0] == y["plane_match"][:, 0]) & (x["plane_match"][:, 0] >= 0))) for x, y in zip(a, b))
    assert kept > 0


def test_deterministic_and_independent_of_the_batch():
    from manhattanslam_amd import plane
    from manhattanslam_amd.match import Matcher
    frames = _ragged()
    caps = (48, 80, 40000)
    a = plane.plane_association_batch(_prm(), frames, caps=caps)
    m = Matcher()
    b = plane.plane_association_batch(_prm(), frames, handle=m, caps=caps)
    parts = plane.plane_association_batch(_prm(), frames[:4], handle=m, caps=caps) + \
        plane.plane_association_batch(_prm(), frames[4:], handle=m, caps=caps)
    m.close()
    for x, y, z in zip(a, b, parts):
        for k in x:
            assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])) and np.array_equal(np.asarray(x[k]), np.asarray(z[k])), k
    _check(frames, a)


def test_device_memory_gives_the_host_bytes():
    import torch
    from manhattanslam_amd import plane
    from manhattanslam_amd.match import Matcher
    frames = _ragged()
    host = plane.plane_association_batch(_prm(), frames)
    caps, arrays, match = plane.pack_associate(frames)
    F, pcap = len(frames), caps[0]
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]
    dm = torch.from_numpy(match).cuda()
    nm = torch.zeros(F, dtype=torch.int32, device="cuda")
    pw = torch.zeros((F, pcap, 12), dtype=torch.float32, device="cuda")
    ph = torch.zeros((F, pcap), dtype=torch.uint8, device="cuda")
    pM = torch.zeros((F, pcap, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    m = Matcher()
    plane.plane_association_device(m, _prm(), F, caps, d, dm, nm, pw, ph, pM)
    m.sync()
    m.close()
    for f, fr in enumerate(frames):
        k = len(fr["plane_coef"])
        assert int(nm[f]) == host[f]["nmatches"]
        assert np.array_equal(dm[f, :k].cpu().numpy(), host[f]["plane_match"])
        assert pw[f, :k].cpu().numpy().tobytes() == host[f]["plane_w"].tobytes()
        assert np.array_equal(ph[f, :k].cpu().numpy(), host[f]["plane_has"])
        assert pM[f, :k].cpu().numpy().tobytes() == host[f]["pM"].tobytes()


@pytest.mark.parametrize("what", ["pcap", "mcap", "ptcap"])
def test_limits_are_refused_without_a_launch(what):
    from manhattanslam_amd import MslError, plane
    fr = sc.room(3050)[0]
    caps = dict(pcap=16, mcap=16, ptcap=4096)
    caps[what] = dict(pcap=65, mcap=4097, ptcap=(1 << 22) + 1)[what]
    named = r"\(-1\): msl_plane_associate: %s %d outside 1 \.\. %d$" % (what, caps[what], caps[what] - 1)
    if what == "ptcap":                                                       # the refusal comes before any staging of the arrays
        from manhattanslam_amd._lib import check, lib, ptr
        (pc, mc, _), arrays, match = plane.pack_associate([fr], 16, 16, 4096)
        out = [np.zeros(1, np.int32), np.zeros((1, 16, 12), np.float32), np.zeros((1, 16), np.uint8), None]
        with pytest.raises(MslError, match=named):
            check(lib.msl_plane_associate_batch(0, 1, pc, mc, caps["ptcap"], ptr(_prm()), *[ptr(a) for a in arrays], 0, ptr(match),
                                                *[ptr(a) for a in out], 0), "msl_plane_associate_batch")
    else:
        with pytest.raises(MslError, match=named):
            plane.plane_association_batch(_prm(), [fr], caps=(caps["pcap"], caps["mcap"], caps["ptcap"]))
    _check([fr], plane.plane_association_batch(_prm(), [fr]))                  # the device is still usable

"""msl_refresh_map_lines on the device against its sequential model (tests/linefuse_model.py::update_average_dir): normals and distances
as bytes for 0, 1, 2, 64, 65 and 300 observations, every status, the in-place table rows; and MapLine::ComputeDistinctiveDescriptors as
msl_refresh_map_points(MSL_REFRESH_DESC) over the line descriptors."""
import numpy as np
import pytest

from tests import linefuse_model as lf
from tests import linefuse_scenes as ls

pytestmark = pytest.mark.gpu
F32 = np.float32
COUNTS = (0, 1, 2, 64, 65, 300)


@pytest.fixture(scope="module")
def matcher():
    from manhattanslam_amd.match import Matcher
    h = Matcher()
    yield h
    h.close()


def _scene():
    """300 keyframes of three keylines around a room, and lines with COUNTS observations plus the exits: a bad line, a reference keyline
    whose octave is outside the pyramid, a reference keyframe that is not among the observations (keyline 0 is read), a reference outside
    the table."""
    from manhattanslam_amd import KEYLINE_DTYPE
    from tests.triangulate_scenes import make_pose
    r = np.random.RandomState(3)
    n_tab = 300
    table = []
    for k in range(n_tab):
        kl = np.zeros(3, KEYLINE_DTYPE)
        kl["octave"] = [k % 8, (k + 3) % 8, 9 if k == 5 else (k + 5) % 8]
        table.append(dict(kl=kl, ldesc=r.randint(0, 256, (3, 32)).astype(np.uint8), Tcw=make_pose(r.uniform(-1, 1, 3), r.uniform(-0.3, 0.3, 3))))
    xyz, obs, ref, flags = [], [], [], []

    def line(n, bad=False, ref_kf=None, idx=None):
        a = r.uniform(-2, 2, 3) + [0, 0, 5]
        xyz.append(np.concatenate([a, a + r.uniform(-0.5, 0.5, 3)]))
        kfs = [int(k) for k in r.permutation(n_tab)[:n]]
        o = [(k, int(r.randint(0, 2)) if idx is None else idx) for k in kfs]
        obs.append(o); flags.append(0 if bad else 1)
        ref.append((o[len(o) // 2][0] if o else 0) if ref_kf is None else ref_kf)
    for n in COUNTS:
        line(n)
    line(4, bad=True)
    obs_5 = len(xyz)
    line(3, idx=2); obs[-1][0] = (5, 2); ref[-1] = 5                              # the reference keyline has octave 9
    line(3); ref[-1] = next(k for k in range(n_tab) if k not in dict(obs[-1]))    # absent: observations[pRefKF] = 0
    line(3, ref_kf=n_tab)                                                         # outside the table
    lines = dict(xyz=np.array(xyz), flags=np.array(flags, np.uint8), ref=np.array(ref, np.int32))
    return table, lines, obs, obs_5


def test_refresh_map_lines_matches_model(matcher):
    from manhattanslam_amd import linefuse, mappoint
    table, lines, obs, i_oct = _scene()
    p = ls.prm()
    rp = mappoint.refresh_params(p["scale_factors"])
    n = len(obs)
    ids = list(range(n))[::-1]                                                    # any order
    want = [lf.update_average_dir(p, table, lines["xyz"][i], obs[i], int(lines["ref"][i]), bad=not lines["flags"][i]) for i in ids]
    st = [w[0] for w in want]
    assert [len(o) for o in obs[:6]] == list(COUNTS)
    assert st[::-1] == [lf.NO_OBS] + [lf.NORMAL_WRITTEN] * 5 + [lf.R_BAD, lf.BAD_OCTAVE, lf.NORMAL_WRITTEN, lf.BAD_OCTAVE]
    rows = dict(ln_normal=np.full((n, 3), 7.25, np.float64), ln_dist=np.full((n, 2), 7.25, F32))
    got = linefuse.refresh_map_lines(rp, table, obs, lines, ids, rows=rows, handle=matcher)
    assert got["status"].tolist() == st
    assert got["out_normal"].tobytes() == np.array([w[1] for w in want]).tobytes()
    assert got["out_dist"].tobytes() == np.array([w[2] for w in want], F32).tobytes()
    for f, i in enumerate(ids):                                                   # rows written only where the status says so
        if st[f] == lf.NORMAL_WRITTEN:
            assert rows["ln_normal"][i].tobytes() == want[f][1].tobytes() and rows["ln_dist"][i].tobytes() == want[f][2].tobytes()
            assert np.isfinite(want[f][1]).all() and 0.9 < np.linalg.norm(want[f][1]) * (1 + 1e-9) and want[f][2][1] > want[f][2][0] > 0
        else:
            assert (rows["ln_normal"][i] == 7.25).all() and (rows["ln_dist"][i] == 7.25).all() and not want[f][1].any() and not want[f][2].any()
    # the _batch form, and without the table rows
    batch = linefuse.refresh_map_lines(rp, table, obs, lines, ids)
    assert all(batch[k].tobytes() == got[k].tobytes() for k in linefuse.REFRESH_OUT_KEYS)


def test_refresh_map_lines_device_memory_and_limits(matcher):
    """Device memory on the handle's stream writes the same bytes and only the rows of ids; limits are refused with nothing written."""
    import torch
    from manhattanslam_amd import linefuse, mappoint
    from manhattanslam_amd._lib import lib, ptr
    table, lines, obs, _ = _scene()
    p = ls.prm()
    rp = mappoint.refresh_params(p["scale_factors"])
    n = len(obs)
    ids = np.array([1, 5, 6, 3], np.int32)
    host = linefuse.refresh_map_lines(rp, table, obs, lines, ids, handle=matcher)
    klcap, t = linefuse.pack_line_table(table)
    o = mappoint.pack_observations(obs)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1) if a.dtype.names else np.ascontiguousarray(a)).cuda()
    d_t = {k: dev(t[k]) for k in linefuse.REFRESH_TABLE_KEYS}; d_o = {k: dev(v) for k, v in o.items()}
    d_l = dict(ln_xyz=dev(lines["xyz"]), ln_flags=dev(lines["flags"]), ln_ref=dev(lines["ref"]))
    out = linefuse.refresh_outputs(len(ids), zeros=lambda shape, dt: torch.zeros(shape, dtype=getattr(torch, np.dtype(dt).name), device="cuda"))
    rows = dict(ln_normal=torch.full((n, 3), 7.25, dtype=torch.float64, device="cuda"), ln_dist=torch.full((n, 2), 7.25, dtype=torch.float32, device="cuda"))
    linefuse.refresh_map_lines_device(matcher, rp, len(table), klcap, n, len(ids), int(o["obs_off"][-1]), d_t, d_o, d_l, dev(ids), out, rows)
    matcher.sync()
    for k in linefuse.REFRESH_OUT_KEYS:
        assert out[k].cpu().numpy().tobytes() == host[k].tobytes(), k
    rn = rows["ln_normal"].cpu().numpy()
    assert rn[1].tobytes() == host["out_normal"][0].tobytes() and rn[5].tobytes() == host["out_normal"][1].tobytes() and (rn[[0, 2, 4, 6, 7, 8, 9]] == 7.25).all()
    fill = lambda shape, dt: np.full(int(np.prod(shape)) * np.dtype(dt).itemsize, 0x5A, np.uint8).view(dt).reshape(shape)

    def call(n_tab=len(table), klcap=klcap, n_lines=n, n_items=len(ids), prm=rp, ids=ids):
        res = linefuse.refresh_outputs(len(ids), zeros=fill)
        rc = lib.msl_refresh_map_lines(matcher.h, n_tab, klcap, n_lines, n_items, int(o["obs_off"][-1]), ptr(prm), *[ptr(t[k]) for k in linefuse.REFRESH_TABLE_KEYS],
                                       *[ptr(o[k]) for k in linefuse.OBS_KEYS], ptr(lines["xyz"]), ptr(lines["flags"]), ptr(lines["ref"]), ptr(ids), 0,
                                       *[ptr(res[k]) for k in linefuse.REFRESH_OUT_KEYS], None, None, 0)
        return rc, all((v.view(np.uint8) == 0x5A).all() for v in res.values())
    assert call() == (0, False)
    for kw, word in ((dict(klcap=257), b"klcap"), (dict(n_tab=4097), b"n_tab"), (dict(n_lines=1048577), b"n_lines"), (dict(n_items=n + 1), b"n_items")):
        assert call(**kw) == (-1, True) and word in lib.msl_last_error(), kw
    q = rp.copy(); q["nlevels"] = 17
    assert call(prm=q) == (-1, True)
    assert call(ids=np.array([1, 1, 2, 3], np.int32)) == (-1, True) and b"twice" in lib.msl_last_error()
    assert call(ids=np.array([1, n, 2, 3], np.int32)) == (-1, True)


def test_line_descriptors_are_refresh_map_points(matcher):
    """MapLine::ComputeDistinctiveDescriptors == msl_refresh_map_points with MSL_REFRESH_DESC alone over mLineDescriptors."""
    from manhattanslam_amd import mappoint
    total = 0
    for name in ls.ALL:
        g, p, cur, targets = ls.graph(name)
        table, lines = g.table(), g.lines()
        obs = [ml.observations() for ml in g.mls]
        ids = [ml.id for ml in g.mls if not ml.bad and ml.obs]
        got = mappoint.refresh_map_points(mappoint.refresh_params(p["scale_factors"]), [dict(desc=k["ldesc"]) for k in table], obs,
                                          dict(flags=lines["flags"]), ids, what=mappoint.REFRESH_DESC, handle=matcher)
        for f, i in enumerate(ids):
            g.mls[i].desc[:] = 0
            g.mls[i].compute_distinctive_descriptors()
            assert got["status"][f] == mappoint.DESC_WRITTEN and got["out_desc"][f].tobytes() == g.mls[i].desc.tobytes(), (name, i)
        total += len(ids)
    assert total > 100

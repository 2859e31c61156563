"""The sequential model of the plane clouds (tests/plane_cloud_model.py) against independent statements of what it pins: exact rational
means, floorf's cells, a least-squares fit, the log form of the RANSAC stop, and the reachability of every status.  CPU only."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import plane_cloud_model as pcm
from tests import plane_cloud_scenes as sc

F32, F64 = np.float32, np.float64


def _cloud(seed, n=3000, span=1.5):
    rng = np.random.default_rng(seed)
    return rng.uniform(-span, span, (n, 3)).astype(F32)


def _groups(pts, leaf=0.2):
    v = pcm.voxel_of(pts, leaf)
    order = sorted(set(map(tuple, v[:, ::-1])))                               # ascending (vz, vy, vx)
    return [(k, np.nonzero(np.all(v[:, ::-1] == k, axis=1))[0]) for k in order]


def test_means_are_the_exact_means_of_the_quantised_coordinates():
    pts = _cloud(1, 800)
    st, out, _ = pcm.voxel_grid(pts, None, 0.2)
    groups = _groups(pts)
    assert st == 0 and len(out) == len(groups) > 100
    for (k, idx), o in zip(groups, out):
        for a in range(3):
            q = [Fraction(int(x)) for x in pcm.quantise(pts[idx, a])]
            mean = sum(q, Fraction(0)) / len(q) / (1 << 24)
            # the model's value is the float32 nearest to the float64 nearest to the exact mean (the sum is below 2^53: exact in double)
            assert o[a] == F32(F64(float(sum(q, Fraction(0)))) / 16777216.0 / F64(len(q)))
            assert abs(Fraction(float(o[a])) - mean) <= Fraction(float(np.spacing(np.abs(o[a])))) / 2 + Fraction(1, 1 << 60)


def test_means_against_the_float64_mean_of_the_original_coordinates():
    """Quantising to 2^-24 m moves a coordinate by at most 2^-25 m, so the mean moves by at most that; then one rounding to float32."""
    pts = _cloud(2, 3000, span=30.0)
    st, out, _ = pcm.voxel_grid(pts, None, 0.2)
    groups = _groups(pts)
    assert st == 0 and len(out) == len(groups)
    for (k, idx), o in zip(groups, out):
        mean = pts[idx].astype(F64).mean(axis=0)
        assert np.all(np.abs(o.astype(F64) - mean) <= 2.0 ** -25 + np.spacing(np.abs(o)).astype(F64) / 2 + 1e-12)


def test_a_shuffled_input_gives_identical_bytes():
    pts = _cloud(3)
    rgb = np.random.default_rng(3).integers(0, 256, (len(pts), 3)).astype(np.uint8)
    a = pcm.voxel_grid(pts, rgb, 0.2)
    for seed in (4, 5):
        p = np.random.default_rng(seed).permutation(len(pts))
        b = pcm.voxel_grid(pts[p], rgb[p], 0.2)
        assert a[0] == b[0] == 0 and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


def test_negative_coordinates_and_cell_faces_follow_floorf():
    inv = F32(1.0) / F32(0.2)
    xs = np.array([-0.0, 0.0, -1e-7, 0.2, -0.2, 0.4, -0.4, 0.6, 1.0, -1.0, 0.19999999, -0.20000002, 3.0000002, -32767.998], F32)
    pts = np.stack([xs, np.zeros_like(xs), np.zeros_like(xs)], axis=1)
    v = pcm.voxel_of(pts, 0.2)[:, 0]
    want = [math.floor(float(F32(x * inv))) for x in xs]                       # the float32 product, then floor
    assert list(v) == want
    assert v[2] == -1 and v[0] == 0 and v[1] == 0 and v[8] == 5 and v[9] == -5 and v[-1] < -163000
    # points on both sides of a face land in two voxels, in ascending order
    st, out, _ = pcm.voxel_grid(np.array([[0.01, 0, 0], [-0.01, 0, 0], [0.0, 0, 0]], F32), None, 0.2)
    assert st == 0 and len(out) == 2 and out[0, 0] < 0 < out[1, 0]


def test_output_order_is_z_then_y_then_x():
    pts = sc.block(3, 2, 2)[::-1].copy()
    st, out, _ = pcm.voxel_grid(pts, None, 0.2)
    v = pcm.voxel_of(out, 0.2)
    keys = [tuple(r[::-1]) for r in v]
    assert st == 0 and keys == sorted(keys) and len(keys) == 12


def test_non_finite_and_far_points_are_skipped():
    pts = np.array([[0.1, 0.1, 0.1], [np.nan, 0, 0], [0, np.inf, 0], [32768.0, 0, 0], [0, 0, -40000.0], [0.15, 0.1, 0.1], [32767.0, 0, 0]], F32)
    st, out, _ = pcm.voxel_grid(pts, None, 0.2)
    assert st == 0 and len(out) == 2 and out[1, 0] == F32(32767.0)


def test_colour_is_the_truncated_float_mean():
    pts = np.full((3, 3), 0.1, F32)
    rgb = np.array([[255, 0, 10], [254, 1, 11], [254, 1, 12]], np.uint8)
    _, _, c = pcm.voxel_grid(pts, rgb, 0.2)
    assert c.tolist() == [[254, 0, 11]]


def test_refit_recovers_an_exact_plane():
    rng = np.random.default_rng(7)
    for normal, d in (((0.0, 0.0, 1.0), -2.0), ((0.6, 0.0, 0.8), -1.5), ((1.0, 2.0, -2.0), 3.0)):
        n = np.asarray(normal, F64) / np.linalg.norm(normal)
        uv = rng.uniform(-1, 1, (500, 2))
        _, a, b = sc._basis(n)
        pts = (-d * n + uv[:, :1] * a + uv[:, 1:] * b).astype(F32)
        got = pcm.refit(pts).astype(F64)
        P = pts.astype(F64)
        c = P.mean(axis=0)
        w, v = np.linalg.eigh((P - c).T @ (P - c))                             # numpy's least-squares plane
        ls = v[:, 0] * np.sign(v[:, 0] @ got[:3])
        assert abs(np.linalg.norm(got[:3]) - 1) < 1e-6
        assert np.max(np.abs(got[:3] - ls)) < 1e-5 and abs(got[3] + ls @ c) < 1e-5
        assert np.max(np.abs(np.abs(got[:3]) - np.abs(n))) < 1e-5 and abs(abs(got[3]) - abs(d)) < 1e-5


def test_tree_sum_is_a_sum():
    x = np.random.default_rng(8).normal(size=(1000, 3))
    assert np.allclose(pcm.tree_sum(x), x.sum(axis=0), rtol=1e-12, atol=1e-12)
    assert pcm.tree_sum(np.zeros((0, 3))).tolist() == [0, 0, 0] and pcm.tree_sum(x[:1]).tolist() == x[0].tolist()


def test_stop_agrees_with_the_log_form_away_from_ties():
    p = 0.99
    checked = 0
    for N in (4, 5, 17, 100, 4096):
        for count in sorted({0, 1, 3, N // 3, N // 2, (2 * N) // 3, N - 1, N}):
            w = count / N
            q = 1.0 - w ** 3
            for it in range(1, 50):
                if q <= 0.0:
                    want = True
                elif q >= 1.0:
                    want = False
                else:
                    k = math.log(1 - p) / math.log(q)                          # PCL: go on while iterations < k
                    if abs(it - k) < 1e-6 * max(1.0, k):
                        continue                                               # a tie: the two forms may round apart
                    want = not it < k
                assert pcm.stop_after(it, count, N, p, 50) == want, (N, count, it)
                checked += 1
    assert checked > 1000
    assert pcm.stop_after(50, 0, 10, p, 50) and not pcm.stop_after(49, 0, 10, p, 50)


def test_sampler_draws_three_distinct_points():
    for N in (4, 5, 100):
        for k in range(40):
            s = pcm.sample3(12345, k, N)
            assert len(set(s)) == 3 and all(0 <= x < N for x in s)
    assert pcm.plane_seed(7, 0) == 7 and pcm.plane_seed(7, 1) != pcm.plane_seed(7, 2)


def test_every_status_is_reachable():
    fr = sc.status_frame()
    assert sc.margins_ok(fr)
    got = pcm.plane_clouds(fr, sc.PRM, 64, 1 << 16)
    assert got["status"].tolist() == [pcm.KEPT, pcm.KEPT, pcm.GATE, pcm.FEW, pcm.FEW, pcm.KEPT, pcm.KEPT, pcm.NO_MODEL, pcm.KEPT, pcm.FEW]
    assert got["plane_src"].tolist() == [0, 1, 5, 6, 8] and got["plane_npts"].tolist()[2:4] == [4, 5]
    assert np.array_equal(np.diff(got["pt_off"]), got["plane_npts"]) and got["pt_off"][-1] == len(got["pts"]) == len(got["rgb"])
    # the sign rule: plane 1's detector normal points the other way, the kept coefficients follow the detector's d
    for k, i in enumerate(got["plane_src"]):
        d0 = pcm.detector_coef(*fr["planes"][i])[3]
        assert d0 * got["plane_coef"][k, 3] > 0
        assert abs(np.linalg.norm(got["plane_coef"][k, :3].astype(F64)) - 1) < 1e-6
    small = pcm.plane_clouds(fr, sc.PRM, 2, 1 << 16)                            # pcap exhausted: the third kept plane and every later one
    assert small["status"].tolist() == [0, 0, pcm.GATE, pcm.FEW, pcm.FEW, pcm.NO_ROOM, pcm.NO_ROOM, pcm.NO_MODEL, pcm.NO_ROOM, pcm.FEW]
    tight = pcm.plane_clouds(fr, sc.PRM, 64, int(got["pt_off"][2]) + 3)         # ptcap exhausted at the four-point plane
    assert tight["status"].tolist()[5:9] == [pcm.NO_ROOM, pcm.NO_ROOM, pcm.NO_MODEL, pcm.NO_ROOM] and tight["n_out"] == 2
    st, _, _ = pcm.voxel_grid(sc.block(16, 16, 16), None, 0.2)
    assert st == 0
    st, _, _ = pcm.voxel_grid(np.concatenate([sc.block(16, 16, 16), sc.block(1, 1, 1, (16, 0, 0))]), None, 0.2)
    assert st == pcm.VOXELS
    st, _, _ = pcm.voxel_grid(np.array([[-30000, -30000, -30000], [30000, 30000, 30000]], F32), None, 0.2)
    assert st == pcm.GRID


def test_merge_statuses_and_layout():
    fr = sc.merge_frame()
    got = pcm.map_plane_merge(fr, sc.PRM, 1 << 16)
    assert got["status"].tolist() == [pcm.MERGED, 0, pcm.MERGED, 0, pcm.MERGED, 0]
    assert got["pt_off"][0] == 0 and np.array_equal(np.diff(got["pt_off"]), [len(c) for c in got["clouds"]])
    for j in (1, 3, 5):
        assert got["clouds"][j].tobytes() == np.asarray(fr["mp_clouds"][j], F32).tobytes()
    # two frame planes into row 0, one after another: the second sees the first's result
    first = pcm.voxel_grid(np.concatenate([pcm.transform(fr["Twc"], fr["clouds"][0]), fr["mp_clouds"][0]]), None, 0.2)[1]
    second = pcm.voxel_grid(np.concatenate([pcm.transform(fr["Twc"], fr["clouds"][3]), first]), None, 0.2)[1]
    assert got["clouds"][0].tobytes() == second.tobytes() and np.all(np.isfinite(second))
    # a new row is the voxel grid of the transformed frame cloud alone
    assert got["clouds"][2].tobytes() == pcm.voxel_grid(pcm.transform(fr["Twc"], fr["clouds"][1]), None, 0.2)[1].tobytes()
    # a failed merge leaves the row as it was; ptcap exhausted empties the rest
    big = dict(clouds=[sc.block(16, 16, 16), sc.block(1, 1, 1)], rgbs=None, merge_into=[0, 0], Twc=sc.IDENTITY,
               mp_clouds=[sc.block(1, 1, 1, (20, 0, 0)), sc.block(2, 1, 1)], mp_rgbs=None)
    g = pcm.map_plane_merge(big, sc.PRM, 1 << 16)
    assert g["status"].tolist() == [pcm.VOXELS, 0] and len(g["clouds"][0]) == 2   # the second merge still ran on the kept cloud
    g = pcm.map_plane_merge(big, sc.PRM, 3)
    assert g["status"].tolist() == [pcm.VOXELS, pcm.NO_ROOM] and g["pt_off"].tolist() == [0, 2, 2]


def test_transform_is_one_rounding_of_the_double_expression():
    T = sc.pose(5)
    p = _cloud(9, 50)
    got = pcm.transform(T, p)
    want = (p.astype(F64) @ T.reshape(3, 4)[:, :3].T + T.reshape(3, 4)[:, 3])
    assert np.max(np.abs(got.astype(F64) - want)) <= np.max(np.spacing(np.abs(got))) and got.dtype == F32
    assert pcm.transform(sc.IDENTITY, p).tobytes() == p.tobytes()


@pytest.mark.parametrize("seed", [31, 32])
def test_scenes_keep_their_margins(seed):
    assert sc.margins_ok(sc.walls_frame(seed, colour=False))

"""Scenes for msl_plane_clouds and msl_map_plane_merge (tests/plane_cloud_model.py is the contract): small frames whose detector planes
cover every status and every small-cloud case, and map merges with shared, new, empty and untouched rows.  Every scene keeps each gate and
inlier decision at least 2^-19 away from its threshold (margins_ok checks it against the model on the CPU)."""
import functools

import numpy as np

from tests import plane_cloud_model as pcm

F32, F64 = np.float32, np.float64
PRM = pcm.params(leaf=0.2, dis_th=0.05, max_iterations=50, probability=0.99)
MARGIN = 2.0 ** -19


def _basis(normal):
    n = np.asarray(normal, F64) / np.linalg.norm(normal)
    a = np.cross(n, [1.0, 0.0, 0.0] if abs(n[0]) < 0.9 else [0.0, 1.0, 0.0])
    a /= np.linalg.norm(a)
    return n, a, np.cross(n, a)


def wall(rng, normal, center, extent, n, noise=0.002):
    """n points of a planar patch (extent: half sizes along the two in-plane axes), float64."""
    nn, a, b = _basis(normal)
    u = rng.uniform(-extent[0], extent[0], n)[:, None]; v = rng.uniform(-extent[1], extent[1], n)[:, None]
    return np.asarray(center, F64) + u * a + v * b + rng.normal(0, noise, n)[:, None] * nn


def cells(rng, cells_xy, z, per_cell=1, jitter=0.03):
    """Points of the plane z = const near the centres of the given (ix, iy) voxel columns (leaf 0.2): one coarse point per cell."""
    out = []
    for ix, iy in cells_xy:
        c = np.array([(ix + 0.5) * 0.2, (iy + 0.5) * 0.2, z])
        out.append(c + np.concatenate([rng.uniform(-jitter, jitter, (per_cell, 2)), rng.normal(0, 0.001, (per_cell, 1))], axis=1))
    return np.concatenate(out)


class Frame:
    def __init__(self, seed, colour):
        self.rng = np.random.default_rng(seed)
        self.pts, self.vertices, self.planes, self.seed, self.colour = [], [], [], seed * 2654435761 & 0xFFFFFFFF, colour
        self.n = 0

    def add(self, pts, normal, center, shuffle=True):
        pts = np.asarray(pts, F64).reshape(-1, 3)
        idx = np.arange(self.n, self.n + len(pts))
        self.pts.append(pts); self.n += len(pts)
        self.vertices.append(np.sort(idx).astype(np.int32))
        n = np.asarray(normal, F64) / np.linalg.norm(normal)
        self.planes.append((n, np.asarray(center, F64)))

    def done(self, pad=7):
        cloud = np.concatenate(self.pts + [np.zeros((pad, 3))]) if self.pts else np.zeros((pad, 3))
        rgb = self.rng.integers(0, 256, (len(cloud), 3)).astype(np.uint8) if self.colour else None
        return dict(cloud=cloud, rgb=rgb, vertices=self.vertices, planes=self.planes, seed=self.seed)


@functools.lru_cache(maxsize=None)
def status_frame(seed=11, colour=True):
    """One frame whose detector planes reach every status but VOXELS, GRID and NO_ROOM: two walls, a gate failure, clouds of 1 (all points
    in one voxel), 3, 4 and 5 coarse points, an all-collinear plane, a wall with NaN and far vertices, and a plane without vertices."""
    fr = Frame(seed, colour)
    rng = fr.rng
    fr.add(wall(rng, (0.1, 0.2, 1.0), (0.3, -0.2, 2.5), (1.2, 0.9), 600), (0.1, 0.2, 1.0), (0.3, -0.2, 2.5))
    fr.add(wall(rng, (1.0, 0.1, -0.3), (-1.5, 0.4, 3.0), (0.8, 1.1), 300), (-1.0, -0.1, 0.3), (-1.5, 0.4, 3.0))      # the detector's normal flipped
    fr.add(wall(rng, (0.0, 1.0, 0.2), (0.0, 1.0, 2.0), (1.0, 0.6), 200), (0.0, 1.0, 0.2), (0.0, 1.5, 2.0))          # gate: the centre 0.5 m off
    fr.add(cells(rng, [(3, 3)], 2.1, per_cell=20), (0, 0, 1), (0.7, 0.7, 2.1))                                      # one voxel
    fr.add(cells(rng, [(0, 0), (2, 1), (1, 3)], 2.1, per_cell=3), (0, 0, 1), (0.3, 0.3, 2.1))                       # three coarse points
    fr.add(cells(rng, [(0, 0), (3, 0), (0, 3), (3, 4)], 1.7, per_cell=2), (0, 0, 1), (0.3, 0.3, 1.7))               # four
    fr.add(cells(rng, [(-4, -2), (-1, -2), (-4, 1), (-2, 2), (-1, 0)], 1.3, per_cell=2), (0, 0, -1), (-0.5, -0.2, 1.3))   # five
    line = np.array([[0.1 + 0.2 * i, 0.5, 2.5] for i in range(6)], F32).astype(F64)                                 # exactly collinear, one per voxel
    fr.add(line, (0, 0, 1), (0.5, 0.5, 2.5))
    bad = wall(rng, (0.3, -1.0, 0.1), (0.5, -1.2, 2.2), (0.9, 0.7), 250)
    bad[::17] = np.nan; bad[5::29, 1] = np.inf; bad[3::31] = [40000.0, 0.0, 1.0]; bad[4::37, 2] = -32768.0
    fr.add(bad, (0.3, -1.0, 0.1), (0.5, -1.2, 2.2))
    fr.add(np.zeros((0, 3)), (0, 0, 1), (0, 0, 1))
    return fr.done()


@functools.lru_cache(maxsize=None)
def walls_frame(seed, n_planes=4, colour=False, n=400):
    fr = Frame(seed, colour)
    rng = fr.rng
    for _ in range(n_planes):
        normal = rng.normal(size=3); center = rng.uniform(-2, 2, 3) + [0, 0, 3]
        fr.add(wall(rng, normal, center, rng.uniform(0.5, 1.5, 2), n), normal, center)
    return fr.done()


def shuffled(fr, seed):
    """The same frame with the vertices of every plane listed in another order."""
    rng = np.random.default_rng(seed)
    return dict(fr, vertices=[rng.permutation(v).astype(np.int32) for v in fr["vertices"]])


def margins_ok(fr, prm=PRM):
    for i, (normal, center) in enumerate(fr["planes"]):
        tr = {}
        pcm.plane_cloud(fr["cloud"], fr.get("rgb"), fr["vertices"][i], normal, center, fr["seed"], i, prm, tr)
        if tr.get("margin", np.inf) < MARGIN:
            return False
    return True


def pose(seed):
    """Twc: 12 doubles, row-major."""
    rng = np.random.default_rng(seed)
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return np.concatenate([R, rng.uniform(-1, 1, (3, 1))], axis=1).reshape(12)


@functools.lru_cache(maxsize=None)
def merge_frame(seed=21, colour=True):
    """Five frame planes and six map rows: rows 0 (a cloud with a NaN and a far point) takes frame planes 0 and 3, row 2 is new (empty) and
    takes plane 1, row 4 takes plane 2, rows 1, 3 (empty) and 5 are untouched, plane 4 merges nowhere."""
    rng = np.random.default_rng(seed)
    cl = lambda n: wall(rng, rng.normal(size=3), rng.uniform(-1, 1, 3) + [0, 0, 2.5], (0.8, 0.6), n, 0.01).astype(F32)
    col = lambda c: rng.integers(0, 256, (len(c), 3)).astype(np.uint8)
    clouds = [cl(90), cl(60), cl(120), cl(75), cl(40)]
    row0 = cl(80); row0[7] = np.nan; row0[11] = [0.0, -50000.0, 1.0]
    mp = [row0, cl(33), np.zeros((0, 3), F32), np.zeros((0, 3), F32), cl(64), cl(17)]
    mp[5][2] = np.nan                                                          # an untouched row is copied bit for bit, NaN included
    fr = dict(clouds=clouds, rgbs=[col(c) for c in clouds] if colour else None, merge_into=[0, 2, 4, 0, -1], Twc=pose(seed), mp_clouds=mp,
              mp_rgbs=[col(c) for c in mp] if colour else None)
    return fr


def block(nx, ny, nz, origin=(0, 0, 0)):
    """One point at the centre of every voxel of an nx x ny x nz block (leaf 0.2), float32."""
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), axis=-1).reshape(-1, 3)
    return ((g + np.asarray(origin) + 0.5) * 0.2).astype(F32)


IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F64)


def check_clouds(frames, got, pcap, ptcap, prm=PRM):
    """Every output of msl_plane_clouds against the model, as bytes."""
    for f, fr in enumerate(frames):
        want = pcm.plane_clouds(fr, prm, pcap, ptcap)
        g = got[f]
        assert g["n_out"] == want["n_out"], (f, g["n_out"], want["n_out"], g["status"], want["status"])
        assert np.array_equal(g["status"], want["status"]), (f, g["status"], want["status"])
        assert np.array_equal(g["plane_src"], want["plane_src"]) and np.array_equal(g["plane_npts"], want["plane_npts"]), f
        assert np.array_equal(g["pt_off"], want["pt_off"]), f
        assert g["pts"].tobytes() == want["pts"].tobytes(), f
        assert g["plane_coef"].tobytes() == want["plane_coef"].tobytes(), (f, g["plane_coef"], want["plane_coef"])
        if fr.get("rgb") is not None:
            assert g["rgb"].tobytes() == want["rgb"].tobytes(), f
    return True


def check_merge(frames, got, ptcap, prm=PRM):
    """Every output of msl_map_plane_merge against the model, as bytes."""
    for f, fr in enumerate(frames):
        want = pcm.map_plane_merge(fr, prm, ptcap)
        g = got[f]
        assert np.array_equal(g["status"], want["status"]), (f, g["status"], want["status"])
        assert np.array_equal(g["pt_off"], want["pt_off"]), (f, g["pt_off"], want["pt_off"])
        for j, (a, b) in enumerate(zip(g["clouds"], want["clouds"])):
            assert a.tobytes() == b.tobytes(), (f, j)
        if want["rgbs"] is not None:
            for j, (a, b) in enumerate(zip(g["rgbs"], want["rgbs"])):
                assert a.tobytes() == b.tobytes(), (f, j)
    return True


# ---- the device-memory form (GPU tests) ---------------------------------------------------------------------------------------------------
def prm_record():
    from manhattanslam_amd import plane_cloud
    return plane_cloud.plane_cloud_params(**PRM)


def dev(a):
    import torch
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype.fields is not None or a.dtype == np.uint32:                    # records and unsigned words travel as bytes
        a = a.view(np.uint8)
    return torch.from_numpy(a).cuda()


def clouds_on_device(frames, pcap, ptcap, fill=0):
    """msl_plane_clouds in device memory; returns the raw output arrays (n_out, coef, npts, src, off, pts, rgb, status) on the host."""
    import torch
    from manhattanslam_amd import plane_cloud
    from manhattanslam_amd.match import Matcher
    V, P, has_rgb, arrays = plane_cloud.pack_clouds(frames)
    F = len(frames)
    d = [dev(a) for a in arrays]
    full = lambda shape, dt: torch.full(shape, fill, dtype=dt, device="cuda")
    outs = [full((F,), torch.int32), full((F, pcap, 4), torch.float32), full((F, pcap), torch.int32), full((F, pcap), torch.int32),
            full((F, pcap + 1), torch.int32), full((F, ptcap, 3), torch.float32), full((F, ptcap, 3), torch.uint8) if has_rgb else None,
            full((F, P), torch.int32)]
    torch.cuda.synchronize()
    m = Matcher()
    plane_cloud.plane_clouds_device(m, prm_record(), F, V, P, pcap, ptcap, d, *outs)
    m.sync()
    m.close()
    return [None if o is None else o.cpu().numpy() for o in outs]


def as_results(frames, raw):
    n_out, coef, npts, src, off, pts, rgb, status = raw
    res = []
    for f, fr in enumerate(frames):
        n = int(n_out[f]); m = int(off[f, n])
        res.append(dict(n_out=n, plane_coef=coef[f, :n], plane_npts=npts[f, :n], plane_src=src[f, :n], pt_off=off[f, :n + 1], pts=pts[f, :m],
                        rgb=None if rgb is None else rgb[f, :m], status=status[f, :len(fr["planes"])]))
    return res

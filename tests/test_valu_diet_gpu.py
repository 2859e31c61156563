"""GPU tests around the kernels whose instruction count was cut without touching an arithmetic expression: kb_seed_plane / kb_seed_finish are
compiled without the SLP vectoriser, k_fast builds its 16-bit pairs with one byte permute each and scores on (r, -r) pairs.  The k_fuse test
pins who reads the screen keys and which launch's keys they must be (a k_fuse that leaves keys only where they are read was measured and not
kept; any such change has to keep this test).  Everything is compared with the CPU oracle bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SURFEL_FIELDS_F = ("px", "py", "pz", "nx", "ny", "nz", "size", "color", "weight")
SURFEL_FIELDS_I = ("r", "g", "b", "updateTimes", "lastUpdate")


def bits(a):
    return a.view(np.int32) if a.dtype.kind == "f" else a


def assert_records_identical(a, b, fields, what):
    assert len(a) == len(b), (what, len(a), len(b))
    for f in fields:
        bad = np.flatnonzero(bits(a[f]) != bits(b[f]))
        if len(bad):
            d = np.abs(a[f][bad].astype(np.float64) - b[f][bad].astype(np.float64))
            print(f"{what}: field {f}: {len(bad)} of {len(a)} records differ, max abs {np.nanmax(d) if len(d) else 0}")
        assert len(bad) == 0, (what, f, len(bad), bad[:10])


# ---- k_fuse: screen keys only where they are read ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def oracle_maps(oracle):
    """{n: the oracle's map after the nine keyframes of tests/fuse_keys_child.py on the n-surfel map}, computed once for both chains"""
    from manhattanslam_amd import synth
    from tests import fuse_keys_child as ch
    from tests.oracle_lib import OracleSurfel
    I = synth.TUM1
    out = {}
    for n in ch.SIZES:
        m, frames = ch.inputs(n)
        o = OracleSurfel(ch.W, ch.H, I["fx"], I["fy"], I["cx"], I["cy"], 30.0, 0.5)
        o.map_set(m)
        for k, (gray, depth, member, pose) in enumerate(frames):
            o.fuse_map(k, gray, depth, member, pose)
        out[n] = o.map_get()
    return out


def run_child(tmp_path, name, **env_set):
    env = {k: v for k, v in os.environ.items() if k not in ("MSL_SF_DEFER", "MSL_SF_DEAL", "MSL_SF_DEAL_EVERY")}
    env.update(env_set)
    out = str(tmp_path / (name + ".npz"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fuse_keys_child.py"), out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fuse_keys_child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    return np.load(out)


@pytest.mark.parametrize("chain", ["classic", "deferred"])
def test_fuse_keys_are_those_of_the_last_keyframe(oracle_maps, tmp_path, chain):
    """One resident call of nine keyframes per map (1 024 surfels = 8 sub-blocks, 8 192 = 64, in k_fuse grids of 128 and 192 sub-blocks: the
    grid covers what the keyframes may spawn; half of each map in view of every keyframe), on the
    classic chain (MSL_SF_DEFER=0) and on deferred windows (=1), each in a child process: the map is the oracle's bit for bit, the dealing
    table is a permutation of the grid, the keys in memory are those of keyframe 8 (the maps alternate sub-blocks only keyframes 0 .. 7 see
    with sub-blocks only keyframe 8 sees, so keys of any earlier launch would be the reverse pattern), and the same call with MSL_SF_DEAL=0
    leaves the identical map.  Threshold 3/4 of the sub-blocks: the right launch gives (nearly) all, an earlier one (nearly) none; a new
    surfel that refills a deleted slot can change a sub-block's side."""
    from tests import fuse_keys_child as ch
    defer = "0" if chain == "classic" else "1"
    dealt, plain = run_child(tmp_path, "dealt", MSL_SF_DEFER=defer), run_child(tmp_path, "plain", MSL_SF_DEFER=defer, MSL_SF_DEAL="0")
    for n in ch.SIZES:
        what = f"{chain} chain, {n} surfels"
        cl, df = (int(x) for x in dealt[f"chain{n}"])
        assert (cl, df) == ((ch.NKF, 0) if chain == "classic" else (1, ch.NKF - 1)), (what, cl, df)   # (the first keyframe after an upload is classic)
        mg = dealt[f"map{n}"]
        assert_records_identical(mg, oracle_maps[n], SURFEL_FIELDS_I + SURFEL_FIELDS_F, what)
        assert mg.tobytes() == plain[f"map{n}"].tobytes(), (what, "MSL_SF_DEAL=0 leaves another map")
        assert int(plain[f"G{n}"]) == 0
        G = int(dealt[f"G{n}"])
        table, keys = dealt[f"table{n}"], dealt[f"keys{n}"]
        assert G >= 8 and G % 8 == 0 and G * 128 >= len(mg), (what, G, len(mg))
        assert np.array_equal(np.sort(table), np.arange(G, dtype=np.uint32)), (what, "the table is not a permutation of the grid")
        nsb = n // 128
        odd, even = keys[1:nsb:2], keys[0:nsb:2]
        print(f"{what}: grid {G}, map {len(mg)}; keys < 255 on {int((odd < 255).sum())} of {len(odd)} odd sub-blocks, = 255 on {int((even >= 255).sum())} of {len(even)} even ones")
        assert (odd < 255).mean() >= 0.75 and (even >= 255).mean() >= 0.75, (what, keys[:nsb])
        for name, d in (("dealt", dealt), ("plain", plain)):   # MSL_SF_DEAL=0: still the keys of the call's last keyframe
            k = d[f"keys{n}"]
            assert (k[1:nsb:2] < 255).mean() >= 0.75 and (k[0:nsb:2] >= 255).mean() >= 0.75, (what, name, k[:nsb])


# ---- kb_seed_plane / kb_seed_finish ----------------------------------------------------------------------------------------------------------

SEED_FIELDS = ("x", "y", "meanIntensity", "size", "normX", "normY", "normZ", "posX", "posY", "posZ", "viewCos", "meanDepth", "r", "g", "b", "fused", "stable", "use")


def plane_frame(k, w, h, intr):
    """A keyframe of the synthetic room (planes, 2 % depth holes) with a rectangular hole and a Huber tail: every 16th pixel moved by up to
    +-0.8 m along its ray, so that seeds have points on both sides of the +-0.4 m band and beyond it."""
    from manhattanslam_amd import synth
    gray, depth, member, pose = synth.surfel_frame(k, w, h, intr=intr, variant="B" if k % 2 else "A")
    rng = np.random.default_rng(1000 + 31 * k + w)
    depth = depth.copy()
    tail = rng.random(depth.shape) < 1.0 / 16
    depth[tail] += rng.uniform(-0.8, 0.8, int(tail.sum())).astype(np.float32)
    depth[depth < 0] = 0.0
    depth[h // 3:h // 3 + max(2, h // 8), w // 4:w // 4 + max(3, w // 6)] = 0.0
    return gray, np.ascontiguousarray(depth), member, pose


@pytest.mark.parametrize("w,h,nkf", [(16, 16, 1), (24, 40, 1), (641, 480, 2)])
def test_seeds_and_fused_map_are_the_oracles_bits(oracle, w, h, nkf):
    """16 x 16 (one 2 x 2 block of seeds), 24 x 40 (a last lattice row and column whose windows are clipped) and 641 x 480 (the STRADDLE
    instantiation, two keyframes): every field of every seed record after the plane fit, and the map after the fusion -- which consumes every
    field of FuseRec (normal, depth, world position, weight, size, intensity, colour, valid) -- equal the oracle's bit for bit."""
    from manhattanslam_amd import SurfelFusion, synth, SURFEL_DTYPE
    from tests.oracle_lib import OracleSurfel
    intr = synth.scaled_intrinsics(synth.TUM1, w)
    g = SurfelFusion(w, h, intr["fx"], intr["fy"], intr["cx"], intr["cy"], 30.0, 0.5)
    o = OracleSurfel(w, h, intr["fx"], intr["fy"], intr["cx"], intr["cy"], 30.0, 0.5)
    m = synth.surfel_map(20000, ref=0).astype(SURFEL_DTYPE)
    g.map_upload(m); o.map_set(m)
    for k in range(nkf):
        gray, depth, member, pose = plane_frame(k, w, h, intr)
        g.fuse_resident(k, gray, depth, member, pose)
        o.fuse_map(k, gray, depth, member, pose)
        assert np.array_equal(g.debug_index(), o.index()), (w, h, k)
        sg, so = g.debug_seeds(), o.seeds()
        assert_records_identical(sg, so, [f for f in SEED_FIELDS if f in sg.dtype.names], f"{w}x{h} seeds of keyframe {k}")
        if w >= 24:
            assert (so["normX"] != 0).sum() > 0, "no seed got a plane"
        assert_records_identical(g.map_download(), o.map_get(), SURFEL_FIELDS_I + SURFEL_FIELDS_F, f"{w}x{h} map after keyframe {k}")
    g.close()


# ---- k_fast -------------------------------------------------------------------------------------------------------------------------------------

def fast_images(w, h):
    rng = np.random.default_rng(w * 7 + h)
    yy, xx = np.mgrid[0:h, 0:w]
    return {"flat": np.full((h, w), 90, np.uint8),                                   # nothing at iniTh: every cell takes the minTh fallback
            "faint": (90 + 9 * (((xx // 5) + (yy // 5)) & 1)).astype(np.uint8),     # corners of contrast 9: none at iniTh = 20, some at minTh = 7
            "checkerboard": (40 + 170 * (((xx // 6) + (yy // 6)) & 1)).astype(np.uint8),
            "noise": rng.integers(0, 256, (h, w), dtype=np.uint8)}


@pytest.mark.parametrize("w,h,levels", [(64, 64, 1), (640, 480, 8)])
def test_fast_keypoints_and_descriptors_are_the_oracles(oracle, w, h, levels):
    """One frame at 64 x 64 (a single FAST cell) and at 640 x 480: an all-flat image and a faint pattern (the minTh fallback), a checkerboard and
    noise give the oracle's keypoints and descriptors."""
    from manhattanslam_amd import ORBextractor
    from tests.test_orb_gpu import _assert_same
    ex = ORBextractor(1000, 1.2, levels, 20, 7, max_width=w, max_height=h)
    oex = oracle.orb_create(1000, 1.2, levels, 20, 7)
    for name, img in fast_images(w, h).items():
        ko, do = oex.extract(img)
        kg, dg = ex(img)
        print(f"{w}x{h} {name}: {len(ko)} keypoints")
        _assert_same(kg, dg, ko, do)
        if name == "flat":
            assert len(ko) == 0
        if name == "noise" or (name == "checkerboard" and w >= 640):
            assert len(ko) > 0
    ex.close()

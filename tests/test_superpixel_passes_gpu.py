"""GPU parity of the superpixel iteration kernels (kb_assign, kb_update_seeds) at the places where their code takes another path: partial waves
and workgroups, ragged rows of dual cells, window quads over the right edge, depth lists longer than the register-resident part of the Newton
walk, Huber tails, seeds without depth, and frames without any depth (the other side of kb_assign's scalar sign test).  Every case: index map equal
to the oracle's, seeds by assert_seeds_close, for single keyframes and for the last keyframe of one batch of two.

The oracle runs once per scene (module cache) and its results are shared by the tests that use the scene."""
import numpy as np
import pytest

from tests.test_surfel_gpu import assert_seeds_close

pytestmark = pytest.mark.gpu

# kb_update_seeds keeps the first NEWTON_RB = 4 blocks of 16 elements of a seed's ordered depth list in registers (msl_sf_sp_seeds.hip)
REG_ELEMS = 16 * 4


def _intr(w):
    from manhattanslam_amd import synth
    return {k: v * (w / 640.0) for k, v in synth.TUM1.items()}


def _flat_frame(w, h, k, depth_of):
    """Uniform grey (+-2) and a depth image given by depth_of(x, y) (metres; 0 = invalid); no plane members."""
    from manhattanslam_amd import synth
    rng = np.random.default_rng(1000 + k)
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    gray = (120 + rng.integers(-2, 3, size=(h, w))).astype(np.uint8)
    depth = np.ascontiguousarray(depth_of(x, y, rng).astype(np.float32))
    member = np.full(((h + 1) // 2, (w + 1) // 2), -1, np.int32)
    return gray, depth, member, synth.camera_pose(k)


LONG_SEED = (4, 4)   # lattice position (x, y) of the seed that owns its whole window in the long-list scenes (72 x 64: a 9 x 8 lattice)


def _long_list_frame(k, step):
    """The eight neighbours of LONG_SEED are unused (their centre pixels are plane members: kb_seed_init gives such a seed use = 0), so every
    free pixel of its 16 x 16 window has it as the only used candidate.  step: the lower rows of the window lie 1.5 m behind the upper ones, so
    the Huber tails sit in the part of the list that is walked in LDS (and, one keyframe later, in the register part as well)."""
    def depth_of(x, y, rng):
        d = 6.0 + rng.uniform(-0.002, 0.002, size=x.shape)
        if step:
            d = np.where(y >= (40 if k == 0 else 31), d + 1.5, d)
        return d
    gray, depth, member, pose = _flat_frame(72, 64, k, depth_of)
    cx, cy = LONG_SEED
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                member[(8 * (cy + dy) + 4) // 2, (8 * (cx + dx) + 4) // 2] = 0
    return gray, depth, member, pose


def _huber_frame(w, h, k):
    """A slanted depth step at 8 m that grows from 0.8 m (top) to 2.4 m (bottom): the inverse depths differ too little for the assignment cost to
    snap superpixels to the edge, so the edge cuts through superpixels at every fraction, the residuals on its minority side lie outside the Huber
    band (0.4 m), and the number of Newton steps differs from seed to seed."""
    def depth_of(x, y, rng):
        d = 8.0 + rng.uniform(-0.002, 0.002, size=x.shape)
        return np.where(x + 0.37 * y > 0.45 * w + 3 * k, d + 0.8 + 1.6 * y / h, d)
    return _flat_frame(w, h, k, depth_of)


def _nodepth_frame(w, h, k):
    """Depth dropout at every seed centre (the fallback search of kb_seed_init), a block of whole superpixels without any valid depth (empty
    lists) and scattered invalid pixels elsewhere."""
    def depth_of(x, y, rng):
        d = 3.0 + 0.01 * x + rng.uniform(-0.002, 0.002, size=x.shape)
        d[(x.astype(int) % 8 == 4) & (y.astype(int) % 8 == 4)] = 0.0
        d[8:40, 16:48] = 0.0
        d[rng.random(x.shape) < 0.05] = 0.0
        return d
    return _flat_frame(w, h, k, depth_of)


def _empty_frame(w, h, k):
    return _flat_frame(w, h, k, lambda x, y, rng: np.zeros_like(x))


def _synth_frame(w, h, k):
    from manhattanslam_amd import synth
    return synth.surfel_frame(k, w, h, intr=_intr(w), variant="B" if k == 1 else "A")


SCENES = {
    "synth_72x64": (72, 64, lambda k: _synth_frame(72, 64, k)),
    "synth_16x16": (16, 16, lambda k: _synth_frame(16, 16, k)),
    "synth_72x80": (72, 80, lambda k: _synth_frame(72, 80, k)),
    "synth_74x66": (74, 66, lambda k: _synth_frame(74, 66, k)),
    "long_flat": (72, 64, lambda k: _long_list_frame(k, False)),
    "long_step": (72, 64, lambda k: _long_list_frame(k, True)),
    "huber_72x64": (72, 64, lambda k: _huber_frame(72, 64, k)),
    "huber_74x66": (74, 66, lambda k: _huber_frame(74, 66, k)),
    "nodepth_72x64": (72, 64, lambda k: _nodepth_frame(72, 64, k)),
    "nodepth_74x66": (74, 66, lambda k: _nodepth_frame(74, 66, k)),
    "empty_72x64": (72, 64, lambda k: _empty_frame(72, 64, k)),
}
_cache = {}


def _map(n=2000):
    from manhattanslam_amd import synth, SURFEL_DTYPE
    return synth.surfel_map(n, ref=0).astype(SURFEL_DTYPE)


def scene(name):
    """(w, h, the two frames, the oracle's (index map, seeds) after keyframe 0 and after keyframe 1 of the sequence); computed once."""
    if name not in _cache:
        from tests.oracle_lib import OracleSurfel
        w, h, make = SCENES[name]
        I = _intr(w)
        o = OracleSurfel(w, h, I["fx"], I["fy"], I["cx"], I["cy"], 30.0, 0.5)
        o.map_set(_map())
        frames = [make(k) for k in range(2)]
        want = []
        for k, f in enumerate(frames):
            o.fuse_map(k, *f)
            idx, seeds = o.index(), o.seeds()
            idx.setflags(write=False); seeds.setflags(write=False)
            want.append((idx, seeds))
        _cache[name] = (w, h, frames, want)
    return _cache[name]


def check_scene(name):
    """Keyframe 0 alone, keyframe 1 behind it, then both in one batch on a fresh handle: index map and seeds against the oracle's."""
    from manhattanslam_amd import SurfelFusion
    w, h, frames, want = scene(name)
    I = _intr(w)
    g = SurfelFusion(w, h, I["fx"], I["fy"], I["cx"], I["cy"], 30.0, 0.5)
    g.map_upload(_map())
    for k, f in enumerate(frames):
        g.fuse_resident(k, *f)
        assert np.array_equal(g.debug_index(), want[k][0]), (name, "single", k)
        assert_seeds_close(g.debug_seeds(), want[k][1])
    g.close()
    g = SurfelFusion(w, h, I["fx"], I["fy"], I["cx"], I["cy"], 30.0, 0.5)
    g.map_upload(_map())
    g.set_batch_capacity(2)
    g.fuse_resident_batch([0, 1], *(np.stack([f[i] for f in frames]) for i in range(3)), [f[3] for f in frames])
    assert np.array_equal(g.debug_index(), want[1][0]), (name, "batch")   # (the debug accessors read the batch's last keyframe)
    assert_seeds_close(g.debug_seeds(), want[1][1])
    g.close()


def owned_depths(name, k, seed):
    """The valid depths (> 0.1, as updateSeeds counts them) of the pixels the oracle's final index map gives to `seed`, in raster order."""
    w, h, frames, want = scene(name)
    idx, seeds = want[k]
    depth, member = frames[k][1], frames[k][2]
    free = np.repeat(np.repeat(member, 2, axis=0), 2, axis=1)[:h, :w] == -1
    own = (idx == seed) & free & (depth > 0.1)
    return depth[own]


def newton_steps(d):
    """Number of Newton steps the Huber refinement of updateSeeds takes on the depth list d (float32 restatement, list order), and whether a
    step met a residual outside the band."""
    d = d.astype(np.float32)
    mean = np.float32(0)
    for v in d: mean = np.float32(mean + v)
    mean = np.float32(mean / np.float32(len(d)))
    tails = False
    for step in range(1, 6):
        r = (mean - d).astype(np.float32)
        inb = (r.astype(np.float64) < 0.4) & (r.astype(np.float64) > -0.4)
        tails |= bool((~inb).any())
        sa = np.float32(0)
        for ri, b in zip(r, inb):
            sa = np.float32(sa + np.float32(2) * ri) if b else np.float32(np.float64(sa) + (0.4 if ri > 0 else -0.4))
        delta = np.float32(-np.float64(sa) / (np.float64(np.float32(2 * int(inb.sum()))) + 10.0))
        mean = np.float32(mean + delta)
        if -0.01 < delta < 0.01: return step, tails
    return 5, tails


@pytest.mark.parametrize("name", ["synth_72x64", "synth_16x16", "synth_72x80"])
def test_partial_waves_and_ragged_dual_cell_rows(oracle, name):
    """72 x 64: a 9 x 8 lattice = 72 seeds, so the last wave and the last workgroup of kb_update_seeds are partly outside it, and 9 rows of dual
    cells (nby): the last wave of a column of kb_assign has cells below the image when it takes 2 or 4 of them; 16 x 16: four seeds and nby = 3;
    72 x 80: nby = 11, a multiple of neither 2, 3 nor 4 (9 and 3 leave no ragged end for waves of three cells)."""
    w, h = SCENES[name][:2]
    nby = ((h - 5) >> 3) + 2
    assert nby == {64: 9, 16: 3, 80: 11}[h] and nby % 2 and nby % 4 and ((w // 8) * (h // 8)) % 16 != 0
    assert h != 80 or nby % 3
    check_scene(name)


def test_straddle_instantiation(oracle):
    """74 x 66: W mod 8 = 2, window quads that stick out over the right edge."""
    assert 74 % 8 in (1, 2, 3)
    check_scene("synth_74x66")


@pytest.mark.parametrize("name", ["long_flat", "long_step"])
def test_depth_list_longer_than_the_register_part(oracle, name):
    """One seed owns (nearly) its whole 16 x 16 window, so its ordered depth list crosses from the register-resident blocks into the part that is
    walked in LDS; with the depth step the Huber tails lie in that part."""
    seed = LONG_SEED[1] * 9 + LONG_SEED[0]
    for k in range(2):
        d = owned_depths(name, k, seed)
        assert len(d) > REG_ELEMS + 16, (name, k, len(d))
        steps, tails = newton_steps(d)
        print(name, "keyframe", k, "owned pixels with depth", len(d), "Newton steps", steps, "tails", tails)
        assert tails == (name == "long_step")
    check_scene(name)


@pytest.mark.parametrize("name", ["huber_72x64", "huber_74x66"])
def test_huber_tails_with_one_three_and_five_newton_steps(oracle, name):
    """A depth step inside superpixels: residuals outside the Huber band, so the tail chain runs; the seeds of the scene take 1, 3 and 5 Newton
    steps (counted on the oracle's index map)."""
    w, h = SCENES[name][:2]
    counts = {}
    for k in range(2):
        for s in range((w // 8) * (h // 8)):
            d = owned_depths(name, k, s)
            if len(d):
                steps, tails = newton_steps(d)
                counts.setdefault(steps, [0, 0])[1 if tails else 0] += 1
    print(name, "Newton steps -> [seeds without tails, with tails]", dict(sorted(counts.items())))
    for steps in (1, 3, 5):
        assert steps in counts, (name, steps, counts)
    assert sum(v[1] for v in counts.values()) >= 4
    check_scene(name)


@pytest.mark.parametrize("name", ["nodepth_72x64", "nodepth_74x66"])
def test_seeds_without_depth(oracle, name):
    """Empty depth lists (whole superpixels without a valid depth) and dropout at every seed centre (the fallback search of kb_seed_init)."""
    w, h, frames, want = scene(name)
    seeds = want[0][1]
    assert int(((seeds["meanDepth"] == 0) & (seeds["use"] != 0)).sum()) >= 4 and int((seeds["meanDepth"] > 0).sum()) >= 20
    check_scene(name)


def test_frame_without_any_depth(oracle):
    """Every candidate record has invDepth = -1: the other side of kb_assign's scalar sign test, for every candidate of every wave."""
    w, h, frames, want = scene("empty_72x64")
    assert not (want[1][1]["meanDepth"] != 0).any()
    check_scene("empty_72x64")

"""GPU: the cheaper float / double forms of the superpixel kernels (manhattanslam_amd/csrc/msl_sf_sp_arith.h) give the bits of the literal ones --
the transposed FP64 group sums of kb_seed_plane and the float Newton quotient of kb_update_seeds through their test hooks, and the whole
superpixel stage against the CPU oracle on depth images built to run the changed paths."""
import functools

import numpy as np
import pytest

from tests import sp_arith_inputs

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@pytest.mark.parametrize("nvals", [4, 10])
def test_transposed_group_sums_have_the_butterflys_bits(nvals):
    """The joint reduction of kb_seed_plane's four Jacobian / ten Hessian sums, on the host program's order-sensitive inputs, against the array model of
    the one-value butterfly: in the lanes the kernel reads (4: lane l reads J_(l >> 2); 10: the matrix the lanes store, Hessian + 5 I)."""
    from manhattanslam_amd import lib
    from manhattanslam_amd._lib import check, ptr
    G = 254   # (not a multiple of the four groups of a wave: the last wave has idle rows)
    x = sp_arith_inputs.group_inputs(G, nvals)
    model = sp_arith_inputs.butterfly(x)                       # [G][nvals][16], the total in every lane
    seq = np.zeros((G, nvals))
    for l in range(16):
        seq = seq + x[:, :, l]
    assert (_bits(seq) != _bits(model[:, :, 0])).mean() > 0.25   # the inputs are sensitive to the order of the additions
    out = np.full((G, 16), np.nan)
    ref = np.full((G, nvals, 16), np.nan)
    check(lib.msl_debug_group_sums(ptr(x), G, nvals, ptr(out), ptr(ref)))
    assert np.array_equal(_bits(ref), _bits(model)), "the device's butterfly against the array model"
    if nvals == 4:
        want = model[:, np.arange(16) >> 2, np.arange(16)]
    else:
        H = {n: model[:, k, 0] for k, n in enumerate(("00", "01", "02", "03", "11", "12", "13", "22", "23", "33"))}
        want = np.stack([H["00"] + 5, H["01"], H["02"], H["03"], H["01"], H["11"] + 5, H["12"], H["13"],
                         H["02"], H["12"], H["22"] + 5, H["23"], H["03"], H["13"], H["23"], H["33"] + 5], axis=1)
    bad = np.argwhere(_bits(out) != _bits(want))
    assert bad.size == 0, (bad[:5], out[tuple(bad[0])], want[tuple(bad[0])])


def test_newton_quotient_in_float_has_the_double_forms_bits():
    """deltaDepth = (float)((double)(-sumA) / ((double)sumB + 10.0)) as one float division: zero, denormal, huge, infinite and NaN numerators against all
    257 denominators, the float form against the literal form evaluated on the device (NaN bits included) and, where the result is a number, against
    the host's double division."""
    from manhattanslam_amd import lib
    from manhattanslam_amd._lib import check, ptr
    edge = np.array([0x00000000, 0x00000001, 0x00000002, 0x007FFFFF, 0x00800000, 0x00800001, 0x3F800000, 0x3F7FFFFF, 0x3F800001, 0x40490FDB,
                     0x7F7FFFFF, 0x7F7FFFFE, 0x7F000000, 0x7F800000, 0x7FC00000, 0x7F800001, 0x7FFFFFFF, 0x7FA55555, 0x7FD55555, 0x3C23D70A,
                     0x41200000, 0x43828000, 0x4B7FFFFF, 0x0A000001, 0x75555555], np.uint32)
    edge = np.concatenate([edge, edge | np.uint32(0x80000000)])
    rng = np.random.default_rng(5)
    sweep = rng.integers(0, 2 ** 32, 200_000, dtype=np.uint64).astype(np.uint32)
    a = np.concatenate([np.repeat(edge, 257), sweep]).view(np.float32)
    inr = np.concatenate([np.tile(np.arange(257, dtype=np.int32), len(edge)), (np.arange(len(sweep)) % 257).astype(np.int32)])
    out = np.zeros(len(a), np.float32)
    lit = np.zeros(len(a), np.float32)
    check(lib.msl_debug_newton_delta(ptr(a), ptr(inr), len(a), ptr(out), ptr(lit)))
    bad = np.flatnonzero(_bits(out) != _bits(lit))
    assert bad.size == 0, [(hex(_bits(a)[i]), int(inr[i]), hex(_bits(out)[i]), hex(_bits(lit)[i])) for i in bad[:5]]
    with np.errstate(all="ignore"):
        host = ((-a).astype(np.float64) / ((2 * inr).astype(np.float32).astype(np.float64) + 10.0)).astype(np.float32)
    num = ~np.isnan(host)
    assert np.isnan(out[~num]).all() and np.array_equal(_bits(out[num]), _bits(host[num]))
    assert np.isnan(a).sum() > 2000 and np.isinf(a).sum() >= 2 * 257 and (np.abs(a[num]) < 1.2e-38).sum() > 2000


# ---- the whole stage ------------------------------------------------------------------------------------------------------------------------
FLAT_SEED = (6, 22)          # lattice position of the seed that is to own a large flat region
ZERO_ROWS, ZERO_COLS = (88, 128), (8, 64)   # a block of zero depth covering whole seeds (5 x 7 cells)


def _step_side(w, h):
    """The far side of the 1 m depth step: a diagonal through the image."""
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    return (u - v) > 60


def _frame(k, w, h, intr):
    from manhattanslam_amd import synth
    gray, depth, member, pose = synth.surfel_frame(k, w=w, h=h, intr=intr, variant="B")   # (2 % dropout)
    depth = depth.copy()
    gray = gray.copy()
    depth[_step_side(w, h) & (depth > 0)] += np.float32(1.0)
    depth[ZERO_ROWS[0]:ZERO_ROWS[1], ZERO_COLS[0]:ZERO_COLS[1]] = 0.0
    # the flat region: one gray level around FLAT_SEED, the centres of its eight neighbours marked with another one -- their seeds start with
    # that intensity, which costs a pixel of the region 120^2 / 100 against at most 2 * 49 / 16 of distance, so the seed in the middle takes every
    # pixel of the region it is a candidate for (|dx|, |dy| < 8)
    cx, cy = 8 * FLAT_SEED[0] + 4, 8 * FLAT_SEED[1] + 4
    gray[cy - 20:cy + 20, cx - 20:cx + 20] = 60
    for dy in (-8, 0, 8):
        for dx in (-8, 0, 8):
            if dx or dy:
                gray[cy + dy - 1:cy + dy + 2, cx + dx - 1:cx + dx + 2] = 180
    return gray, np.ascontiguousarray(depth), member, pose


@functools.lru_cache(maxsize=None)
def _case(w, h):
    """Inputs and the oracle's results for one image size, computed once: three keyframes, a local map; the oracle after the first keyframe through the
    host-vector call and after all three on a resident map."""
    from manhattanslam_amd import synth, SURFEL_DTYPE
    from tests import oracle_lib
    oracle_lib.load()
    intr = synth.scaled_intrinsics(synth.TUM1, w)
    frames = [_frame(3 + k, w, h, intr) for k in range(3)]
    local = synth.surfel_map(20000, ref=3).astype(SURFEL_DTYPE)
    o = oracle_lib.OracleSurfel(w, h, intr["fx"], intr["fy"], intr["cx"], intr["cy"], 30.0, 0.5)
    gray, depth, member, pose = frames[0]
    lo, no = o.fuse(3, gray, depth, member, pose, local)
    first = dict(local=lo, new=no, index=o.index().copy(), seeds=o.seeds().copy())
    o.map_set(local)
    for k, f in enumerate(frames):
        o.fuse_map(3 + k, f[0], f[1], f[2], f[3])
    batch = dict(map=o.map_get(), index=o.index().copy(), seeds=o.seeds().copy())
    return intr, frames, local, first, batch


def _assert_seeds(got, want, what):
    """Every field of every seed, bit for bit.  (The plane fit adds its FP64 sums lane-wise where the oracle walks the points left to right; on these
    inputs the difference vanishes in the rounding to float -- all fields were bit-equal with the parent commit's kernels as well, so none needs the
    tolerance tests/test_surfel_gpu.py allows.)"""
    for f in want.dtype.names:
        if f.startswith("_"):
            continue
        a, b = got[f], want[f]
        bad = np.flatnonzero(_bits(a) != _bits(b)) if a.dtype.kind == "f" else np.flatnonzero(a != b)
        assert bad.size == 0, (what, f, len(bad), bad[:10], a[bad[:3]], b[bad[:3]])
    fit = (want["normX"] != 0) | (want["normY"] != 0) | (want["normZ"] != 0)
    assert fit.sum() > 300 and (~fit & (want["use"] == 1)).sum() > 10, what   # seeds with a plane fit, and used seeds whose fit did not run


@pytest.mark.parametrize("w,h", [(324, 244), (333, 251), (322, 246)])
def test_superpixel_stage_on_steps_holes_and_a_large_flat_seed(w, h):
    """324x244, 333x251 and 322x246 through fuseInitializeMap and a 3-keyframe fuse_resident_batch.  (322: W mod 8 = 2, the STRADDLE instantiation of
    kb_update_seeds and kb_seed_plane -- a window quad sticks out over the right edge for W mod 8 in {1, 2, 3}; 333 mod 8 = 5 runs the plain one with a
    strip right of the last cell.)  The depth images carry a 1 m step on a diagonal (Huber tails in the seed update, a changing in-band set in the plane
    fit), a block of zero depth over whole seeds (seeds, candidates and pixels without depth), 2 % dropout, and a flat one-coloured region one seed takes
    over (more than 96 valid pixels: the plane fit's rounds beyond its register-resident ones, the seed update's blocks beyond NEWTON_RB)."""
    from manhattanslam_amd import SurfelFusion
    from tests.test_surfel_gpu import assert_surfels_close
    intr, frames, local, first, batch = _case(w, h)
    gray, depth, member, pose = frames[0]
    # from the inputs alone: seed windows (16 x 16 around the lattice centre) that hold both sides of the step, with valid depth, on free pixels
    side = _step_side(w, h)
    free = np.repeat(np.repeat(member, 2, axis=0), 2, axis=1)[:h, :w] == -1
    both = 0
    for sy in range(h // 8):
        for sx in range(w // 8):
            win = (slice(max(8 * sy - 4, 0), 8 * sy + 12), slice(max(8 * sx - 4, 0), 8 * sx + 12))
            ok = free[win] & (depth[win] > 0.1)
            both += int((ok & side[win]).sum() >= 32 and (ok & ~side[win]).sum() >= 32)
    assert both >= 8, both
    near = depth[~side & (depth > 0)]
    assert np.all(depth[side & (depth > 0)] > 1.0) and near.min() > 0.1
    assert not depth[ZERO_ROWS[0]:ZERO_ROWS[1], ZERO_COLS[0]:ZERO_COLS[1]].any() and ZERO_ROWS[0] % 8 == 0 and ZERO_COLS[0] % 8 == 0
    assert free[ZERO_ROWS[0]:ZERO_ROWS[1], ZERO_COLS[0]:ZERO_COLS[1]].all()
    flat = FLAT_SEED[1] * (w // 8) + FLAT_SEED[0]
    owned = first["index"].reshape(h, w) == flat
    assert (owned & (depth > 0.1)).sum() > 96, (owned & (depth > 0.1)).sum()      # (the oracle's index map: the region does what it was built for)
    assert (first["seeds"]["meanDepth"] == 0).sum() > 0 and (first["seeds"]["use"] == 1).sum() > 500

    g = SurfelFusion(w, h, intr["fx"], intr["fy"], intr["cx"], intr["cy"], 30.0, 0.5)
    lg = local.copy()
    ng = g.fuseInitializeMap(3, gray, depth, member, pose, lg)
    assert np.array_equal(g.debug_index(), first["index"])
    _assert_seeds(g.debug_seeds(), first["seeds"], "first keyframe")
    assert_surfels_close(lg, first["local"], "local")
    assert_surfels_close(ng, first["new"], "new")
    g.map_upload(local)
    g.set_batch_capacity(3)
    g.fuse_resident_batch([3, 4, 5], np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]), np.stack([f[2] for f in frames]), [f[3] for f in frames])
    assert_surfels_close(g.map_download(), batch["map"], "resident map")
    assert np.array_equal(g.debug_index(), batch["index"])
    _assert_seeds(g.debug_seeds(), batch["seeds"], "third keyframe of the batch")
    g.close()

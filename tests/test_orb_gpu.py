"""GPU parity: HIP ORB extractor (through the C ABI) vs the CPU oracle, bit-exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _assert_same(kg, dg, ko, do):
    assert len(kg) == len(ko), (len(kg), len(ko))
    for f in ("x", "y", "size", "angle", "response", "octave", "class_id"):
        a, b = kg[f], ko[f]
        assert np.array_equal(a.view(np.int32) if a.dtype.kind == "f" else a,
                              b.view(np.int32) if b.dtype.kind == "f" else b), f
    if len(kg):
        assert np.array_equal(dg, do)
    else:
        assert dg is None or len(dg) == 0


@pytest.fixture(scope="module")
def gpu_orb():
    from manhattanslam_amd import ORBextractor
    ex = ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=8)
    yield ex
    ex.close()


def test_stages_match_oracle(gpu_orb, oracle):
    """Pyramid levels, FAST candidates (order included) and blurred levels are byte-identical."""
    from manhattanslam_amd import synth
    img = synth.orb_frame()
    oex = oracle.orb_create()
    ko, do = oex.extract(img)
    kg, dg = gpu_orb(img)
    for l in range(8):
        if l > 0:
            assert np.array_equal(gpu_orb.debug_level(0, l), oex.level(l)), f"pyramid level {l}"
        assert np.array_equal(gpu_orb.debug_candidates(0, l), oex.candidates(l)), f"candidates level {l}"
        assert np.array_equal(gpu_orb.debug_level(0, l, blurred=True), oex.level(l, blurred=True)), f"blur level {l}"
    _assert_same(kg, dg, ko, do)


@pytest.mark.parametrize("seed_off", [1, 2, 3])
def test_full_extract_bit_exact(gpu_orb, oracle, seed_off):
    from manhattanslam_amd import synth
    img = synth.orb_frame(synth.ORB_SEED + seed_off)
    ko, do = oracle.orb_create().extract(img)
    kg, dg = gpu_orb(img)
    _assert_same(kg, dg, ko, do)
    assert len(kg) >= 1000


def test_batch_matches_single(gpu_orb, oracle):
    from manhattanslam_amd import synth
    imgs = synth.orb_frames(8, seed=77)
    res = gpu_orb.extract_batch(imgs)
    oex = oracle.orb_create()
    for f in range(8):
        ko, do = oex.extract(imgs[f])
        _assert_same(res[f][0], res[f][1], ko, do)


def test_edge_cases(gpu_orb, oracle):
    # constant image: no corners at all -> zero keypoints, descriptors released
    flat = np.full((480, 640), 90, np.uint8)
    k, d = gpu_orb(flat)
    assert len(k) == 0 and d is None
    # empty image: silent return (src/ORBextractor.cc:815-816)
    k, d = gpu_orb(np.zeros((0, 0), np.uint8))
    assert len(k) == 0 and d is None
    # pure noise: far more candidates than quota on every level
    rng = np.random.default_rng(5)
    noise = rng.integers(0, 256, (480, 640), dtype=np.uint8)
    ko, do = oracle.orb_create().extract(noise)
    kg, dg = gpu_orb(noise)
    _assert_same(kg, dg, ko, do)
    # strided input (row stride > width)
    big = np.zeros((480, 700), np.uint8)
    from manhattanslam_amd import synth
    big[:, :640] = synth.orb_frame(1234)
    view = big[:, :640]
    ko, do = oracle.orb_create().extract(np.ascontiguousarray(view))
    kg, dg = gpu_orb(view)
    _assert_same(kg, dg, ko, do)


def test_scale_tables_match_oracle(oracle):
    """a13: the getters of include/ORBextractor.h:58-80 (f32 cumulative products of src/ORBextractor.cc:416-430) and
    mnFeaturesPerLevel (:433-445), bit for bit, for the default and two other parameter sets."""
    from manhattanslam_amd import ORBextractor
    for nf, sc, nl in ((1000, 1.2, 8), (500, 1.2, 6), (2000, 1.5, 5)):
        ex = ORBextractor(nf, sc, nl, 20, 7)
        sf, isf, s2, is2, per, _ = oracle.orb_create(nf, sc, nl, 20, 7).tables()
        for got, want in ((ex.GetScaleFactors(), sf), (ex.GetInverseScaleFactors(), isf), (ex.GetScaleSigmaSquares(), s2),
                          (ex.GetInverseScaleSigmaSquares(), is2)):
            assert np.array_equal(got.view(np.int32), want.view(np.int32))
        assert np.array_equal(ex.features_per_level(), per) and ex.GetLevels() == nl
        assert np.float32(ex.GetScaleFactor()) == np.float32(sc) and ex.capacity == nf + 2 * nl
        ex.close()
    ex = ORBextractor(1000, 1.2, 8, 20, 7)
    assert list(ex.features_per_level()) == [217, 181, 151, 126, 105, 87, 73, 60]
    ex.close()


def test_other_sizes_and_params(oracle):
    """Smaller frame, fewer features/levels, other thresholds."""
    from manhattanslam_amd import ORBextractor, synth
    img = synth.orb_frame(42, 400, 304)
    ex = ORBextractor(500, 1.2, 6, 25, 9, max_width=400, max_height=304)
    ko, do = oracle.orb_create(500, 1.2, 6, 25, 9).extract(img)
    kg, dg = ex(img)
    _assert_same(kg, dg, ko, do)
    ex.close()
    img = synth.orb_frame(43, 1280, 960)
    ex = ORBextractor(1000, 1.2, 8, 20, 7, max_width=1280, max_height=960)
    ko, do = oracle.orb_create().extract(img)
    kg, dg = ex(img)
    _assert_same(kg, dg, ko, do)
    ex.close()


def test_feature_budgets_size_the_quadtree(oracle):
    """The quadtree kernel's node arrays (dynamic LDS) follow the per-level feature budget: a large budget (more than the default dynamic LDS of a
    launch), a budget below four root children, and the default give the oracle's keypoints; low thresholds so that the budgets are reached."""
    from manhattanslam_amd import ORBextractor, synth
    img = synth.orb_frame(77)
    for nf, ini, mn in ((4000, 7, 5), (3000, 20, 7), (40, 20, 7), (24, 20, 7)):
        ex = ORBextractor(nf, 1.2, 8, ini, mn)
        ko, do = oracle.orb_create(nf, 1.2, 8, ini, mn).extract(img)
        kg, dg = ex(img)
        _assert_same(kg, dg, ko, do)
        assert len(kg) > 0
        ex.close()


@pytest.mark.parametrize("w,h,nf,levels,scale", [(640, 160, 137, 4, 1.2), (1280, 200, 1000, 5, 1.2), (640, 480, 60, 12, 1.1), (960, 200, 2000, 3, 1.5),
                                                 (400, 304, 24, 1, 1.2), (1279, 333, 777, 8, 1.2), (1600, 230, 300, 6, 1.2)])
def test_quadtree_node_bound_over_geometries(oracle, w, h, nf, levels, scale):
    """The quadtree's node arrays are sized analytically (max(quota, 4 nIni) + 2 per level): wide images (nIni = round(width / height) up to 8 root
    nodes; tall ones have nIni = 0, which the reference itself cannot handle), tiny and large budgets, 1 to 12 levels, low thresholds so that every
    level reaches its quota.  1600 x 230 with 300 features returns MORE than nfeatures + 2 levels keypoints (the first quadtree round alone makes
    up to 4 nIni nodes per level): the extractor's capacity follows its creation geometry.  An overrun would zero a level (device error); the
    outputs must be the oracle's, bit for bit."""
    from manhattanslam_amd import ORBextractor, synth
    k = max(-(-w // 640), -(-h // 480))
    img = synth.orb_frame(300 + w + nf, 640 * k, 480 * k)[:h, :w].copy()          # the generator makes 4:3 frames: crop one
    ex = ORBextractor(nf, scale, levels, 9, 5, max_width=w, max_height=h)
    ko, do = oracle.orb_create(nf, scale, levels, 9, 5).extract(img)
    kg, dg = ex(img)          # raises on a device-side bound error
    _assert_same(kg, dg, ko, do)
    assert len(kg) >= min(nf, 20) and ex.capacity >= max(len(kg), nf + 2 * levels)
    ex.close()



def test_one_extractor_across_frame_sizes():
    """Frame size A, then B, then A on ONE extractor: its geometry buffers are released and rebuilt at every change (the pinned staging of the
    single-frame call and the frame epilogue's buffers stay), and every result -- the single-frame call and the batched frame epilogue -- is that of
    a fresh extractor created for the size.  (The sizes share one aspect ratio: the keypoint capacity of the first fits the second.)"""
    from manhattanslam_amd import ORBextractor, frame_params, synth
    I = synth.TUM1
    ex = ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=2)
    for w, h in ((640, 480), (480, 360), (640, 480)):
        imgs = synth.orb_frames(2, seed=700 + w, w=w, h=h)
        depths = np.stack([synth.surfel_frame(k, w=w, h=h)[1] for k in range(2)])
        params = frame_params(I["fx"], I["fy"], I["cx"], I["cy"], 40.0, w, h)
        fresh = ORBextractor(1000, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=2)
        kg, dg = ex(imgs[0])
        kf, df = fresh(imgs[0])
        assert len(kg) > 100
        _assert_same(kg, dg, kf, df)
        for got, want in zip(ex.extract_frames(imgs, depths, params), fresh.extract_frames(imgs, depths, params)):
            _assert_same(got[0], got[1], want[0], want[1])
            assert all(x.tobytes() == y.tobytes() for x, y in zip(got[2:], want[2:]))
        fresh.close()
    ex.close()

# The smallest geometry the extractor accepts with two levels: 96 x 80 at scale 1.2 makes level 1 80 x 67, both axes above the 62 px one 30-px FAST
# cell needs; low thresholds so that both levels return keypoints.
_SMALL = dict(w=96, h=80, args=(100, 1.2, 2, 7, 5))


def _small_frames(n=3):
    from manhattanslam_amd import synth
    full = synth.orb_frame(4100)          # (the generator needs room for its rectangles: cut the small frames out of one 640 x 480 frame)
    imgs = np.stack([full[60 + 90 * i:60 + 90 * i + _SMALL["h"], 100 + 150 * i:100 + 150 * i + _SMALL["w"]] for i in range(n)])
    rng = np.random.default_rng(41)
    depths = rng.uniform(0.5, 4.0, imgs.shape).astype(np.float32)
    depths[rng.random(imgs.shape) < 0.2] = 0.0          # pixels without depth
    return imgs, depths


def test_copy_out_paths_are_the_direct_path():
    """Host or device frames in (padded or tightly packed), host or device arrays out, rows of the handle's capacity or longer ones: every way
    through msl_orb_extract_batch and msl_orb_extract_frame_batch gives the bytes of the direct device path and of the single-frame call, and
    the slots of a longer row beyond the capacity are not written."""
    import torch
    from manhattanslam_amd import ORBextractor, frame_params, synth
    from manhattanslam_amd._lib import MSL_MEM_DEVICE, MSL_MEM_HOST, check, lib, ptr
    W, H, B = _SMALL["w"], _SMALL["h"], 3
    imgs, depths = _small_frames(B)
    I = synth.TUM1
    params = frame_params(I["fx"] * W / 640, I["fy"] * H / 480, I["cx"] * W / 640, I["cy"] * H / 480, 40.0, W, H)
    ex = ORBextractor(*_SMALL["args"], max_width=W, max_height=H, max_batch=B)
    C = ex.capacity
    single = [ex(imgs[f]) for f in range(B)]
    assert all(len(k) > 0 for k, _ in single) and all(set(k["octave"]) == {0, 1} for k, _ in single)
    # padded host input: rows of W + 13 bytes, frames 2 rows further apart than they are long
    rs, fs = W + 13, (W + 13) * (H + 2)
    padded = np.full(B * fs, 0xCD, np.uint8)
    dpad = np.full(B * fs, -7.0, np.float32)
    for f in range(B):
        padded[f * fs:f * fs + rs * H].reshape(H, rs)[:, :W] = imgs[f]
        dpad[f * fs:f * fs + rs * H].reshape(H, rs)[:, :W] = depths[f]
    elem = (("kps", 28), ("desc", 32), ("un", 8), ("dep", 4), ("ur", 4), ("cell", 4))
    FILL = 0xA5

    def run(frame, dev, cap, pad):
        names = elem if frame else elem[:2]
        mem = MSL_MEM_DEVICE if dev else MSL_MEM_HOST
        if dev:
            out = {k: torch.full((B, cap * b), FILL, dtype=torch.uint8, device="cuda") for k, b in names}
            n = torch.full((B,), -1, dtype=torch.int32, device="cuda")
            g, d = torch.from_numpy(imgs).cuda(), torch.from_numpy(depths).cuda()
            torch.cuda.synchronize()          # the prefill runs on torch's stream, the extractor on its own
        else:
            out = {k: np.full((B, cap * b), FILL, np.uint8) for k, b in names}
            n = np.full(B, -1, np.int32)
            g, d = (padded, dpad) if pad else (imgs, depths)
        grs, gfs = (rs, fs) if pad else (W, W * H)
        if frame:
            check(lib.msl_orb_extract_frame_batch(ex._h, ptr(g), ptr(d), B, W, H, grs, gfs, 4 * grs, 4 * gfs, mem, ptr(params), ptr(out["kps"]), ptr(out["desc"]),
                                                  ptr(out["un"]), ptr(out["dep"]), ptr(out["ur"]), ptr(out["cell"]), cap, ptr(n), mem), "msl_orb_extract_frame_batch")
        else:
            check(lib.msl_orb_extract_batch(ex._h, ptr(g), B, W, H, grs, gfs, mem, ptr(out["kps"]), ptr(out["desc"]), cap, ptr(n), mem), "msl_orb_extract_batch")
        ex.sync()
        if dev:
            out = {k: v.cpu().numpy() for k, v in out.items()}
            n = n.cpu().numpy()
        return n, out

    for frame in (False, True):
        cases = {"a": run(frame, False, C + 7, True), "b": run(frame, False, C, False), "c": run(frame, True, C, False), "d": run(frame, True, C + 7, False)}
        n0, direct = cases["c"]
        assert (n0 > 0).all()
        for f in range(B):
            ks, ds = single[f]
            assert n0[f] == len(ks) and direct["kps"][f, :28 * n0[f]].tobytes() == ks.tobytes() and direct["desc"][f, :32 * n0[f]].tobytes() == ds.tobytes()
        for name, (n, out) in cases.items():
            cap = C + 7 if name in "ad" else C
            assert n.tobytes() == n0.tobytes(), (frame, name)
            for k, b in (elem if frame else elem[:2]):
                for f in range(B):
                    assert out[k][f, :b * n[f]].tobytes() == direct[k][f, :b * n[f]].tobytes(), (frame, name, k, f)
                assert (out[k][:, b * C:b * cap] == FILL).all(), (frame, name, k)          # beyond the capacity: the caller's prefill
    ex.close()


def test_rejected_size_leaves_the_handle_intact():
    """A frame size the geometry plan rejects (70 x 64: level 1 is 58 x 53, too small for one 30-px FAST cell) costs the handle nothing: the
    geometry it had, its level sizes and its results stay."""
    import ctypes as C
    from manhattanslam_amd import ORBextractor, KEYPOINT_DTYPE
    from manhattanslam_amd._lib import lib, ptr
    W, H = _SMALL["w"], _SMALL["h"]
    img = _small_frames(1)[0][0]
    ex = ORBextractor(*_SMALL["args"], max_width=W, max_height=H, max_batch=3)
    sizes = [ex.level_size(l) for l in range(2)]
    assert sizes == [(96, 80), (80, 67)]
    k0, d0 = ex(img)
    assert len(k0) > 0
    small = np.ascontiguousarray(img[:64, :70])
    kps = np.zeros(ex.capacity, KEYPOINT_DTYPE); desc = np.zeros((ex.capacity, 32), np.uint8); n = C.c_int(-1)
    rc = lib.msl_orb_extract(ex._h, ptr(small), 70, 64, 70, ptr(kps), ptr(desc), ex.capacity, C.byref(n))
    assert rc == -1 and "level 1 (58x53) is too small for the 30-px FAST grid" in lib.msl_last_error().decode()          # MSL_ERR_INVALID
    assert [ex.level_size(l) for l in range(2)] == sizes
    k1, d1 = ex(img)
    assert k1.tobytes() == k0.tobytes() and d1.tobytes() == d0.tobytes()
    ex.close()


def test_device_resident_batch(oracle):
    """Asynchronous batch path with inputs and outputs resident in HBM (the bench.py path)."""
    import torch
    from manhattanslam_amd import ORBextractor, synth, KEYPOINT_DTYPE
    B = 5
    imgs = synth.orb_frames(B, seed=901)
    ex = ORBextractor(1000, 1.2, 8, 20, 7, max_batch=B)
    d_img = torch.from_numpy(imgs).cuda()
    cap = ex.capacity
    d_kps = torch.zeros(B * cap * 28, dtype=torch.uint8, device="cuda")
    d_desc = torch.zeros(B * cap * 32, dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    ex.extract_batch_device(d_img, d_kps, d_desc, d_n, B, 640, 480)
    ex.sync()
    n = d_n.cpu().numpy()
    kps = d_kps.cpu().numpy().view(KEYPOINT_DTYPE).reshape(B, cap)
    desc = d_desc.cpu().numpy().reshape(B, cap, 32)
    oex = oracle.orb_create()
    for f in range(B):
        ko, do = oex.extract(imgs[f])
        _assert_same(kps[f, :n[f]], desc[f, :n[f]], ko, do)
    ex.close()


@pytest.mark.parametrize("dist", [False, True])
def test_frame_epilogue_matches_oracle(oracle, dist):
    """UndistortKeyPoints + ComputeStereoFromRGBD + AssignFeaturesToGrid fused behind the extraction."""
    from manhattanslam_amd import ORBextractor, frame_params, synth
    from tests import oracle_lib
    I = synth.TUM1
    kw = dict(k1=0.262383, k2=-0.953104, p1=-0.005358, p2=0.002628, k3=1.163314) if dist else {}   # Example/TUM1.yaml:13-17
    pg = frame_params(I["fx"], I["fy"], I["cx"], I["cy"], 40.0, 640, 480, **kw)
    po = oracle_lib.frame_params(I["fx"], I["fy"], I["cx"], I["cy"], 40.0, 640, 480, **kw)
    assert pg.tobytes() == po.tobytes()                       # ComputeImageBounds
    if dist:
        assert pg["minX"][0] != 0 and pg["maxX"][0] != 640
    imgs = synth.orb_frames(3, seed=555)
    depths = np.stack([synth.surfel_frame(k)[1] for k in range(3)])
    ex = ORBextractor(1000, 1.2, 8, 20, 7, max_batch=3)
    res = ex.extract_frames(imgs, depths, pg)
    oex = oracle.orb_create()
    for f in range(3):
        ko, do = oex.extract(imgs[f])
        kg, dg, un, dep, ur, cell = res[f]
        _assert_same(kg, dg, ko, do)
        uo, depo, uro, cello = oracle_lib.frame_epilogue(po, ko, depths[f])
        assert un.tobytes() == uo.tobytes() and dep.tobytes() == depo.tobytes() and ur.tobytes() == uro.tobytes()
        assert np.array_equal(cell, cello)
        assert (dep == -1).sum() > 0 and (dep > 0).sum() > 900 and (cell >= 0).sum() > 900
        if dist:
            assert np.abs(un - np.stack([kg["x"], kg["y"]], 1)).max() > 1.0      # the distortion really moves points
    ex.close()


def test_second_gaussian_generation_variant_library():
    """The product built with MSL_BLUR_VARIANT=1 (manhattanslam_amd/variants/libmsl_blur1.so) against the oracle built the same way:
    blurred levels byte-identical, full extraction bit-exact, and different from the default kernel's descriptors."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "manhattanslam_amd", "variants", "libmsl_blur1.so")
    olib = os.path.join(root, "oracle", "libmsl_oracle_blur1.so")
    assert os.path.exists(lib) and os.path.exists(olib), "python -c 'import __graft_entry__ as g; g.build()' builds both variants"
    script = (
        "import numpy as np, sys\n"
        "sys.path.insert(0, %r)\n"
        "from manhattanslam_amd import ORBextractor, synth\n"
        "from tests import oracle_lib\n"
        "o = oracle_lib.load()\n"
        "assert list(o.gaussian_kernel()) == [18, 34, 48, 56, 48, 34, 18]\n"
        "img = synth.orb_frame(synth.ORB_SEED + 4)\n"
        "ex = ORBextractor(1000, 1.2, 8, 20, 7)\n"
        "kg, dg = ex(img)\n"
        "oe = o.orb_create()\n"
        "ko, do = oe.extract(img)\n"
        "assert kg.tobytes() == ko.tobytes() and np.array_equal(dg, do)\n"
        "for l in (0, 3, 7):\n"
        "    assert np.array_equal(ex.debug_level(0, l, blurred=True), oe.level(l, blurred=True))\n"
        "print('variant ok', len(kg))\n" % root)
    env = dict(os.environ, MSL_LIB=lib, MSL_ORACLE_LIB=olib)
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "variant ok" in r.stdout, r.stdout + r.stderr


def test_pyramid_fused_and_per_level_launches_agree(oracle):
    """k_pyramid (all levels in one launch, tiles chained through LDS) is the default; MSL_ORB_PYRAMID=levels keeps one k_resize launch per
    level (also the fallback when a tile chain does not fit the LDS).  Both give the oracle's levels, at several geometries."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = (
        "import numpy as np, sys\n"
        "sys.path.insert(0, %r)\n"
        "from manhattanslam_amd import ORBextractor, synth\n"
        "from tests import oracle_lib\n"
        "o = oracle_lib.load()\n"
        "for (w, h, nl, sf) in ((640, 480, 8, 1.2), (1280, 960, 8, 1.2), (752, 480, 5, 1.5), (320, 240, 12, 1.1), (480, 360, 3, 2.0)):\n"
        "    img = synth.orb_frame(synth.ORB_SEED + 9, w, h)\n"
        "    ex = ORBextractor(800, sf, nl, 20, 7, max_width=w, max_height=h)\n"
        "    kg, dg = ex(img)\n"
        "    oe = o.orb_create(800, sf, nl, 20, 7)\n"
        "    ko, do = oe.extract(img)\n"
        "    for l in range(1, nl):\n"
        "        assert np.array_equal(ex.debug_level(0, l), oe.level(l)), (w, h, l)\n"
        "    assert kg.tobytes() == ko.tobytes() and np.array_equal(dg, do), (w, h)\n"
        "print('pyramid ok')\n" % root)
    for mode in ("fused", "levels"):
        env = dict(os.environ, MSL_ORB_PYRAMID=mode)
        r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0 and "pyramid ok" in r.stdout, mode + "\n" + r.stdout + r.stderr

"""GPU: the map-exchange calls of one surfel handle chained without a pause (upload, resident batches, append, detach, snapshot, restore), the
host-vector mirror across them, and snapshots of maps with wide records -- on small images (64x48: 48 seeds; 72x56: 63), against the CPU oracle.
All comparisons are byte equality or assert_surfels_close."""
import ctypes as C

import numpy as np
import pytest

from tests.test_surfel_gpu import assert_surfels_close, _mk

pytestmark = pytest.mark.gpu

SIZES = [(64, 48), (72, 56)]


def _intr(w):
    from manhattanslam_amd import synth
    return {k: v * (w / 640.0) for k, v in synth.TUM1.items()}


def _frames(w, h, ks):
    from manhattanslam_amd import synth
    fr = [synth.surfel_frame(k, w, h, intr=_intr(w), variant="B" if k % 4 == 1 else "A") for k in ks]
    return np.stack([f[0] for f in fr]), np.stack([f[1] for f in fr]), np.stack([f[2] for f in fr]), [f[3] for f in fr]


_chain_ref = {}


def _chain_reference(w, h):
    """The chain of test_one_chain on the oracle, computed once per image size: the steps, and the oracle's map after each."""
    if (w, h) in _chain_ref:
        return _chain_ref[(w, h)]
    from manhattanslam_amd import synth, SURFEL_DTYPE
    from tests.oracle_lib import OracleSurfel, load, _p
    d = load().dll
    d.mslo_map_detach.restype = C.c_size_t; d.mslo_map_detach.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    I = _intr(w)
    o = OracleSurfel(w, h, I["fx"], I["fy"], I["cx"], I["cy"], 30.0, 0.5)
    nseeds = (w // 8) * (h // 8)
    m0 = synth.surfel_map(20000, ref=0, min_update_times=1).astype(SURFEL_DTYPE)
    extra = synth.surfel_map(50000, ref=2, seed=5, min_update_times=1).astype(SURFEL_DTYPE)   # pushes the map past the 65 536 surfels a new handle holds
    steps, maps, ref = [], [], [0]

    def batch(n):
        refs = list(range(ref[0], ref[0] + n)); ref[0] += n
        args = _frames(w, h, [3 * r for r in refs])
        for j, r in enumerate(refs):
            o.fuse_map(r, args[0][j], args[1][j], args[2][j], args[3][j])
        steps.append(("batch", refs, args)); maps.append(o.map_get().copy())

    o.map_set(m0); steps.append(("upload", m0)); maps.append(m0.copy())
    batch(3)
    assert len(maps[-1]) + len(extra) + nseeds > 65536                    # the append reallocates the map and keeps what is there
    cur = np.concatenate([maps[-1], extra]); o.map_set(cur); steps.append(("append", extra)); maps.append(cur.copy())
    batch(3)
    cur = maps[-1].copy(); buf = np.zeros(len(cur), SURFEL_DTYPE)
    k = d.mslo_map_detach(_p(cur), len(cur), 5, _p(buf))                    # the surfels keyframe 5 updated last
    assert 0 < k < len(cur)
    o.map_set(cur); steps.append(("detach", 5, buf[:k].copy())); maps.append(cur.copy())
    batch(2)
    snap = maps[-1].copy(); steps.append(("snapshot",)); maps.append(snap)
    batch(2)
    assert len(maps[-1]) != len(snap)
    o.map_set(snap); steps.append(("restore",)); maps.append(snap.copy())
    batch(2)
    small = m0[:3000].copy()
    steps.append(("upload", small)); maps.append(small)
    steps.append(("restore",)); maps.append(snap.copy())                    # a restore over a live map smaller than the snapshot
    _chain_ref[(w, h)] = (steps, maps)
    return steps, maps


@pytest.mark.parametrize("one_stream", [False, True])
@pytest.mark.parametrize("w,h", SIZES)
def test_one_chain_of_map_exchange_calls(oracle, w, h, one_stream):
    """upload -> batch of 3 -> append (map_realloc keeping the map) -> batch of 3 -> detach -> batch of 2 -> snapshot -> batch of 2 -> restore ->
    batch of 2, then an upload of a smaller map and a restore, on ONE handle: once comparing the map with the oracle after every step, once without
    any call between the steps (deferred windows and live-count snapshots still pending when the map is replaced; the map compared at the end of
    the chain and after the last restore).  On the handle's own streams and on a single caller stream."""
    import torch
    from manhattanslam_amd import SurfelFusion
    steps, maps = _chain_reference(w, h)
    I = _intr(w)
    stream = torch.cuda.Stream() if one_stream else None
    for check_each in (True, False):
        g = SurfelFusion(w, h, I["fx"], I["fy"], I["cx"], I["cy"], 30.0, 0.5)
        if one_stream:
            g.set_stream(stream.cuda_stream)
        g.set_batch_capacity(3)
        for i, (st, want) in enumerate(zip(steps, maps)):
            if st[0] == "upload":
                g.map_upload(st[1])
            elif st[0] == "batch":
                g.fuse_resident_batch(st[1], *st[2])
            elif st[0] == "append":
                g.map_append(st[1])
            elif st[0] == "detach":
                got = g.map_detach(st[1])
                assert_surfels_close(got, st[2], f"step {i}: detached surfels")
            elif st[0] == "snapshot":
                g.map_snapshot()
            else:
                g.map_restore()
            if check_each or i >= len(steps) - 3:      # (the end of the chain proper, and what follows it)
                assert_surfels_close(g.map_download(), want, f"step {i} ({st[0]}), {w}x{h}, one_stream={one_stream}, check_each={check_each}")
        g.close()


@pytest.mark.parametrize("between", ["batch", "append", "detach", "restore"])
@pytest.mark.parametrize("w,h", SIZES)
def test_mirror_is_dropped_by_every_map_call_in_between(oracle, w, h, between):
    """msl_sf_fuse_ex keeps the device map as the mirror of the caller's vector; a resident batch, map_append, map_detach or map_restore on the same
    handle in between replaces or edits that map, so MSL_SF_LOCAL_UNCHANGED on the next call must be ignored: the vector -- which the test has edited
    as well -- is uploaded again and the edit is seen."""
    from manhattanslam_amd import synth, SURFEL_DTYPE
    I = _intr(w)
    g, o = _mk(I, w, h)
    m = synth.surfel_map(12000, ref=0, min_update_times=1).astype(SURFEL_DTYPE)
    g.map_upload(m[:5000]); g.map_snapshot()                               # (something to restore)
    f0, f1 = (synth.surfel_frame(k, w, h, intr=I) for k in (0, 1))
    lg, lo = m.copy(), m.copy()
    lo, no = o.fuse(0, *f0, lo)
    ng = g.fuseInitializeMap(0, *f0, lg)
    assert_surfels_close(lg, lo, "first call"); assert_surfels_close(ng, no, "first call, new")
    if between == "batch":
        g.fuse_resident(1, *f1)
    elif between == "append":
        g.map_append(m[:700])
    elif between == "detach":
        assert len(g.map_detach(0)) > 0
    else:
        g.map_restore()
    plain, _ = o.fuse(1, *f1, lo.copy())
    seen = np.flatnonzero(plain["lastUpdate"] == 1)[:400]                  # surfels keyframe 1 fuses: the edit moves them out of its range
    assert len(seen) > 50
    lg["pz"][seen] += 50.0; lo["pz"][seen] += 50.0
    lo, no = o.fuse(1, *f1, lo)
    assert not np.array_equal(lo["lastUpdate"], plain["lastUpdate"])       # (the edit shows in the result)
    ng = g.fuseInitializeMap(1, *f1, lg, local_unchanged=True)
    assert_surfels_close(lg, lo, f"hint after {between}"); assert_surfels_close(ng, no, f"hint after {between}, new")
    # and with nothing in between the hint holds: the same call again, on the vector as the call above left it
    lo, no = o.fuse(2, *f1, lo)
    ng = g.fuseInitializeMap(2, *f1, lg, local_unchanged=True)
    assert_surfels_close(lg, lo, "hint honoured"); assert_surfels_close(ng, no, "hint honoured, new")
    g.close()


@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_snapshot_of_wide_records_at_the_layout_boundary(oracle, n):
    """Snapshot and restore of a map whose r, g, b and whose updateTimes / lastUpdate need the wide side arrays, at the 4096-surfel boundary of the
    store layout: the snapshot store is laid out for 4096 or 8192 surfels (12 288 once a larger snapshot has been taken), the live map for 65 536.
    The download after the restore is the uploaded map byte for byte, also from a second snapshot taken of the restored map."""
    from manhattanslam_amd import synth, SURFEL_DTYPE
    g, _ = _mk(_intr(64), 64, 48)
    rng = np.random.default_rng(n)
    m = synth.surfel_map(n, ref=2000000, min_update_times=1).astype(SURFEL_DTYPE)      # lastUpdate around two million: wide hot records
    wide = rng.choice(n, n // 3, replace=False)
    m["r"][wide] = rng.integers(-2**31, 2**31 - 1, len(wide)); m["g"][wide[::2]] = 256; m["b"][wide[::3]] = -1
    m["updateTimes"][wide[::4]] = rng.integers(2048, 5000, len(wide[::4]))
    m["r"][n - 1] = -7; m["lastUpdate"][n - 1] = -(1 << 21); m["r"][0] = 1 << 20      # the first and the last record are wide in both planes
    narrow = synth.surfel_map(9000, ref=2, min_update_times=1).astype(SURFEL_DTYPE)
    for first_bigger in (False, True):
        if first_bigger:
            g.map_upload(narrow); g.map_snapshot()                          # the snapshot store grows to 12 288 surfels and stays there
        g.map_upload(m)
        g.map_snapshot()
        for _ in range(2):
            g.map_upload(narrow[:100])                                      # a fresh map: no wide records
            assert g.map_download().tobytes() == narrow[:100].tobytes()
            g.map_restore()
            assert g.map_size() == n
            assert g.map_download().tobytes() == m.tobytes(), (n, first_bigger)
            g.map_snapshot()                                                # of the restored map: its wide flags came back with it
    g.close()


@pytest.mark.parametrize("w,h", SIZES)
def test_restore_regrows_a_map_snapshotted_at_its_capacity(oracle, w, h):
    """msl_sf_map_restore's grow-again branch: a snapshot taken of a map that has filled its allocation to within one keyframe's seeds (a far-away
    map of 65 536 - 2 * nseeds surfels, two keyframes that only spawn) no longer leaves the room for a keyframe that every map operation keeps,
    so the restore reallocates the map first.  The restored map is the snapshotted one byte for byte, and fusion goes on from it as on the oracle."""
    from manhattanslam_amd import synth, SURFEL_DTYPE
    I = _intr(w)
    g, o = _mk(I, w, h)
    nseeds = (w // 8) * (h // 8)
    far = synth.surfel_map(65536 - 2 * nseeds, ref=0, min_update_times=5).astype(SURFEL_DTYPE)
    far["px"] += 100.0; far["py"] += 100.0; far["pz"] += 100.0
    g.set_batch_capacity(2)
    g.map_upload(far); o.map_set(far)
    a = _frames(w, h, [0, 40])
    g.fuse_resident_batch([0, 1], *a)
    for j in range(2):
        o.fuse_map(j, a[0][j], a[1][j], a[2][j], a[3][j])
    full = g.map_download()
    assert_surfels_close(full, o.map_get(), "map at its capacity")
    assert 65536 - nseeds < len(full) <= 65536
    g.map_snapshot()
    g.map_upload(far[:3000])
    g.map_restore()
    assert g.map_download().tobytes() == full.tobytes()
    b = _frames(w, h, [80, 120])
    g.fuse_resident_batch([2, 3], *b)
    o.map_set(full)
    for j in range(2):
        o.fuse_map(2 + j, b[0][j], b[1][j], b[2][j], b[3][j])
    assert_surfels_close(g.map_download(), o.map_get(), "two keyframes on the regrown map")
    g.close()

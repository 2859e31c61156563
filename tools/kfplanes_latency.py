"""Latency of msl_keyframe_planes and msl_manhattan_observe in device memory on one matcher handle, by event pairs on the handle's stream
(the method of tools/keyframe_latency.py): keyframes of 64 planes over a map of 4096 rows and tables of 65536 entries, one keyframe and a
batch of 8.  msl_keyframe_planes with half of the planes held and half new.  msl_manhattan_observe with 64 distinct held rows, normals on
three axes (a third of the triples pass) and normals so short that every triple passes (41 664 triples, 2 016 pairs: the most), into empty
tables and into tables that hold 20 000 foreign keys.  Both entries edit their tables in place, so every call starts from a device copy of
the pristine arrays, made on the same stream before the first event.  One JSON line per measurement: the median, minimum and 90th
percentile of `reps` calls in microseconds."""
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from manhattanslam_amd import kfplanes, plane
from manhattanslam_amd.match import Matcher

PCAP, MCAP, FCAP, QCAP, KCAP, TH = 64, 4096, 65536, 65536, 4096, 0.1


def keyframe_of(seed, short, prefill, n_held=PCAP):
    """One keyframe of 64 planes, the first n_held on distinct rows of a map of 4096 - (64 - n_held) rows."""
    rng = np.random.default_rng(seed)
    n_map = MCAP - (PCAP - n_held)
    axes = np.eye(3)[np.arange(PCAP) % 3] + rng.normal(0, 0.01, (PCAP, 3))
    coef = np.concatenate([axes * (0.05 if short else 1.0), rng.uniform(-3, 3, (PCAP, 1))], 1).astype(np.float32)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    match = np.full((PCAP, 3), -1, np.int32)
    match[:n_held, 0] = rng.permutation(n_map)[:n_held]
    held = match[:n_held, 0]
    tabs = {}
    for w, name in ((3, "full"), (2, "part")):
        keys = np.sort(rng.integers(0, MCAP, (prefill * 11 // 10, w)), 1)
        keys = np.unique(keys[(np.diff(keys, axis=1) > 0).all(1) & ~np.isin(keys, held).all(1)], axis=0)[:prefill]
        tabs[name] = np.concatenate([keys, np.ones((len(keys), w + 1), np.int64)], 1).astype(np.int32)
    return dict(kf_slot=seed % KCAP, kf_id=seed, plane_coef=coef, plane_npts=rng.integers(50, 500, PCAP).astype(np.int32),
                Tcw=np.concatenate([q * np.sign(np.linalg.det(q)), rng.uniform(-1, 1, (3, 1))], 1).astype(np.float32).reshape(12), plane_match=match,
                plane_outlier=np.zeros((PCAP, 3), np.uint8), mp_w=rng.normal(size=(n_map, 4)).astype(np.float32), mp_flags=np.ones(n_map, np.uint8),
                mp_first_kf=rng.integers(0, 50, n_map).astype(np.int32), full=tabs["full"], part=tabs["part"], kf_Rwc=np.zeros((0, 9), np.float32),
                kf_coef=[], kf_npts=[])


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32).reshape(len(a), -1) if a.dtype.fields is not None else a).cuda()


def timed(stream, reset, fn, reps):
    for _ in range(3):
        reset(); fn()
    stream.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reset()
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    out.sort()
    return dict(med_us=round(out[len(out) // 2], 1), min_us=round(out[0], 1), p90_us=round(out[int(len(out) * 0.9)], 1))


def main(reps=30):
    prm = plane.plane_params(0.2, 0.9, 0.08, 0.9, TH)
    s = torch.cuda.Stream()
    m = Matcher()
    m.set_stream(s.cuda_stream)
    z = lambda shape, dt: torch.zeros(shape, dtype=getattr(torch, np.dtype(dt).name), device="cuda")
    for F in (1, 8):
        with torch.cuda.stream(s):
            _, a = kfplanes.pack([keyframe_of(10 + f, False, 0, n_held=32) for f in range(F)], PCAP, MCAP, FCAP, QCAP, KCAP)
            d, keep = {k: dev(v) for k, v in a.items()}, dev(a["n_map"])
            po = kfplanes.planes_outputs(F, PCAP, z)
            r = timed(s, lambda: d["n_map"].copy_(keep), lambda: kfplanes.keyframe_planes_device(m, F, PCAP, MCAP, KCAP, kfplanes.KEYFRAME, d, po), reps)
            print(json.dumps(dict(what="msl_keyframe_planes", frames=F, planes=PCAP, new=int(po["n_new"].sum()), **r)), flush=True)
            for short in (False, True):
                for prefill in (0, 20000):
                    _, a = kfplanes.pack([keyframe_of(20 + f, short, prefill) for f in range(F)], PCAP, MCAP, FCAP, QCAP, KCAP)
                    d = {k: dev(v) for k, v in a.items()}
                    d["kf_plane_match"] = d["plane_match"]
                    keep = {k: d[k].clone() for k in kfplanes.OBSERVE_INOUT_KEYS}
                    oo = kfplanes.observe_outputs(F, PCAP, z)

                    def reset():
                        for k, v in keep.items():
                            d[k].copy_(v)
                    r = timed(s, reset, lambda: kfplanes.manhattan_observe_device(m, prm, F, PCAP, MCAP, FCAP, QCAP, KCAP, d, oo), reps)
                    print(json.dumps(dict(what="msl_manhattan_observe", frames=F, planes=PCAP, gate="all pass" if short else "three axes",
                                          old_full=int(a["n_full"].sum()), old_part=int(a["n_part"].sum()), added_full=int(oo["added_full"].sum()),
                                          added_part=int(oo["added_part"].sum()), status=int(oo["status"].max()), **r)), flush=True)
    m.sync()
    m.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 30)

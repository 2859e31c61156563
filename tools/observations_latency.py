"""Latency of msl_observations_apply in device memory on one matcher handle, by event pairs on the handle's stream (the method of
tools/keyframe_latency.py), beside the path it replaces, taken with the same timer: the CSR table rebuilt by numpy on the host and the three
arrays copied to the device.  Two maps -- 1 048 576 rows and 65 536 rows with 4 observations each -- and a log of 2 000 ops in the mix of
the fusion replay (7 ADD to 3 REPLACE).  Every repetition starts from the same tables: the in-place arrays are restored outside the event
pair.  The host path is given what an integrator has after its own replay -- the new lists of the touched rows, read here from the
device's result -- and does what is left: new offsets, the shifted copy of every untouched range, the touched ranges, three uploads; its
result is compared with the device's.  One JSON line per measurement: the median, minimum and 90th percentile of `reps` calls in
microseconds."""
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from manhattanslam_amd import observations as ob
from manhattanslam_amd.match import Matcher

N_OPS, PER_ROW, SPARE = 2000, 4, 64


def build(n_pts, n_tab, seed=1):
    """n_pts rows of 4 observations: row p observes keyframes j * n_tab / 4 + p % (n_tab / 4), j = 0 .. 3, at keypoint p // (n_tab / 4), and
    the keyframe holds it there; SPARE free keypoints per keyframe behind them take the ADDs."""
    rng = np.random.default_rng(seed)
    q = n_tab // PER_ROW
    used = n_pts // q
    cap = used + SPARE
    p = np.arange(n_pts, dtype=np.int32)
    kf = (np.arange(PER_ROW, dtype=np.int32)[None, :] * q + (p % q)[:, None]).astype(np.int32)
    idx = np.repeat((p // q)[:, None], PER_ROW, 1).astype(np.int32)
    held = np.full((n_tab, cap), -1, np.int32)
    held[kf.reshape(-1), idx.reshape(-1)] = np.repeat(p, PER_ROW)
    uright = np.where(rng.random((n_tab, cap)) < 0.6, 10.0, -1.0).astype(np.float32)
    t = dict(n_kps=np.full(n_tab, cap, np.int32), uright=uright, obs_off=(np.arange(n_pts + 1) * PER_ROW).astype(np.int32), obs_kf=kf.reshape(-1),
             obs_idx=idx.reshape(-1), held_id=held, pt_flags=np.ones(n_pts, np.uint8),
             pt_nobs=np.where(uright[kf, idx] >= 0, 2, 1).sum(1).astype(np.int32), pt_ref=kf[:, 0].copy(),
             pt_found=rng.integers(1, 9, n_pts).astype(np.int32), pt_visible=rng.integers(9, 30, n_pts).astype(np.int32),
             pt_replaced=np.full(n_pts, -1, np.int32))
    ops, free = [], np.full(n_tab, used, np.int32)
    while len(ops) < N_OPS:
        a = int(rng.integers(0, n_pts))
        if rng.random() < 0.7:
            k = int(rng.integers(0, n_tab))
            if free[k] < cap:
                ops.append((ob.ADD, a, k, int(free[k])))
                free[k] += 1
        else:
            ops.append((ob.REPLACE, a, int(rng.integers(0, n_pts))))
    t["ops"] = ob.pack_ops(ops)
    return t, cap


def host_rebuild(t, touched, lists, pinned, dev):
    """The new table from the old one and the new (keyframe, keypoint) lists of the touched rows, then the three uploads."""
    off = t["obs_off"]
    length = np.diff(off)
    length[touched] = [len(x) for x in lists]
    new_off = np.zeros(len(off), np.int32)
    np.cumsum(length, out=new_off[1:])
    keep = np.ones(len(off) - 1, bool)
    keep[touched] = False
    rows = np.repeat(np.arange(len(off) - 1, dtype=np.int32), np.diff(off))
    sel = keep[rows]
    dest = (np.arange(off[-1], dtype=np.int32) + (new_off[:-1] - off[:-1])[rows])[sel]
    pinned["obs_kf"][dest], pinned["obs_idx"][dest] = t["obs_kf"][sel], t["obs_idx"][sel]
    for p, x in zip(touched, lists):
        pinned["obs_kf"][new_off[p]:new_off[p + 1]], pinned["obs_idx"][new_off[p]:new_off[p + 1]] = x[:, 0], x[:, 1]
    pinned["obs_off"][:] = new_off
    for k in ("obs_off", "obs_kf", "obs_idx"):
        dev[k].copy_(torch.from_numpy(pinned[k]), non_blocking=True)
    return int(new_off[-1])


def percentiles(out):
    out.sort()
    return dict(med_us=round(out[len(out) // 2], 1), min_us=round(out[0], 1), p90_us=round(out[int(len(out) * 0.9)], 1))


def main(reps=30):
    s = torch.cuda.Stream()
    m = Matcher()
    m.set_stream(s.cuda_stream)
    lib = os.environ.get("MSL_LIB", "product")
    for n_pts, n_tab in ((1 << 20, 2048), (1 << 16, 256)):
        t, cap = build(n_pts, n_tab)
        n_obs, ocap, tcap = n_pts * PER_ROW, n_pts * PER_ROW + N_OPS, 2 * N_OPS
        with torch.cuda.stream(s):
            dev = lambda a: torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).cuda()
            d = {k: dev(v) for k, v in t.items()}
            entry = {k: d[k].clone() for k in ob.INOUT_KEYS}
            out = ob.outputs(n_pts, N_OPS, ocap, tcap, lambda shape, dt: torch.zeros(shape, dtype=getattr(torch, np.dtype(dt).name), device="cuda"))
            times = []
            for rep in range(reps + 5):                                   # five warm-up calls (the first grows the handle's scratch)
                for k in ob.INOUT_KEYS:
                    d[k].copy_(entry[k])
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(s)
                ob.apply_device(m, n_tab, cap, n_pts, n_obs, N_OPS, ocap, tcap, d, d, out)
                b.record(s)
                b.synchronize()
                if rep >= 5:
                    times.append(a.elapsed_time(b) * 1e3)
            counts = out["counts"].cpu().numpy()
            print(json.dumps(dict(what="msl_observations_apply", rows=n_pts, observations=n_obs, ops=N_OPS, new_total=int(counts[0]),
                                  touched=int(counts[1]), too_long=int(counts[2]), turned_bad=int(counts[3]), lib=lib, **percentiles(times))), flush=True)
            got = {k: out[k].cpu().numpy() for k in ("obs_off_out", "obs_kf_out", "obs_idx_out", "touched")}
            touched = got["touched"][:counts[1]]
            lists = [np.stack([got["obs_kf_out"][got["obs_off_out"][p]:got["obs_off_out"][p + 1]],
                               got["obs_idx_out"][got["obs_off_out"][p]:got["obs_off_out"][p + 1]]], 1) for p in touched]
            pinned = dict(obs_off=np.zeros(n_pts + 1, np.int32), obs_kf=np.zeros(ocap, np.int32), obs_idx=np.zeros(ocap, np.int32))
            pinned = {k: torch.from_numpy(v).pin_memory().numpy() for k, v in pinned.items()}
            up = {k: torch.zeros(len(v), dtype=torch.int32, device="cuda") for k, v in pinned.items()}
            times = []
            for rep in range(reps + 5):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(s)
                total = host_rebuild(t, touched, lists, pinned, up)
                b.record(s)
                b.synchronize()
                if rep >= 5:
                    times.append(a.elapsed_time(b) * 1e3)
            same = total == counts[0] and all(np.array_equal(up[k].cpu().numpy()[:n], got[k + "_out"][:n])
                                             for k, n in (("obs_off", n_pts + 1), ("obs_kf", total), ("obs_idx", total)))
            print(json.dumps(dict(what="host rebuild + upload", rows=n_pts, observations=n_obs, ops=N_OPS, bytes=int(4 * (n_pts + 1 + 2 * total)),
                                  equals_device=bool(same), lib=lib, **percentiles(times))), flush=True)
    m.sync()
    m.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 30)

"""Latency of msl_connections_apply in device memory on one matcher handle, by event pairs on the handle's stream (the method of
tools/observations_latency.py): one log of two UPDATE and three KF_BAD ops on a graph of 200 keyframes, alone and behind the
msl_covisibility call that produces its two weight rows.  The map is 20 000 points, each observed by four keyframes of a sliding window
of 12, so a keyframe is connected to 19 others on average at th = 15; the graph on entry is the library's own: msl_covisibility of every
keyframe and one log of 199 UPDATE ops (every keyframe but the new one).  Every repetition starts from that graph: the in-place arrays
are restored outside the event pair.  One JSON line per measurement: the median, minimum and 90th percentile of `reps` calls in microseconds."""
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from manhattanslam_amd import connections as cn, mappoint
from manhattanslam_amd.match import Matcher

N_TAB, N_PTS, CAP, TH, WINDOW = 200, 20000, 1024, 15, 12


def build(seed=1):
    rng = np.random.default_rng(seed)
    held, n_kps, obs = np.full((N_TAB, CAP), -1, np.int32), np.zeros(N_TAB, np.int32), []
    for p in range(N_PTS):
        lo = min(p * N_TAB // N_PTS, N_TAB - WINDOW)
        ks = sorted(int(k) for k in lo + rng.permutation(WINDOW)[:4])
        obs.append([(k, int(n_kps[k])) for k in ks])
        for k in ks:
            held[k, n_kps[k]] = p
            n_kps[k] += 1
    assert n_kps.max() <= CAP
    return held, n_kps, mappoint.pack_observations(obs)


def percentiles(out):
    out.sort()
    return dict(med_us=round(out[len(out) // 2], 1), min_us=round(out[0], 1), p90_us=round(out[int(len(out) * 0.9)], 1))


def main(reps=30):
    s = torch.cuda.Stream()
    m = Matcher()
    m.set_stream(s.cuda_stream)
    lib = os.environ.get("MSL_LIB", "product")
    held, n_kps, o = build()
    n_obs = int(o["obs_off"][-1])
    with torch.cuda.stream(s):
        dev = lambda a: torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).cuda()
        zeros = lambda shape, dt: torch.zeros(shape, dtype=getattr(torch, np.dtype(dt).name), device="cuda")
        t = dict(held_id=dev(held), n_kps=dev(n_kps), pt_flags=dev(np.ones(N_PTS, np.uint8)), obs_off=dev(o["obs_off"]), obs_kf=dev(o["obs_kf"]))

        def covisibility(kfs, out):
            mappoint.covisibility_device(m, N_TAB, CAP, N_PTS, len(kfs), n_obs, N_TAB, TH, t["held_id"], t["n_kps"], t["pt_flags"], t["obs_off"], t["obs_kf"],
                                         dev(np.array(kfs, np.int32)), out)

        # the graph on entry: every keyframe but the last connected in creation order
        g = dict(cw=zeros((N_TAB, N_TAB), np.int32), conn=dev(np.full((N_TAB, N_TAB), -1, np.int32)), conn_w=zeros((N_TAB, N_TAB), np.int32),
                 n_conn=zeros((N_TAB,), np.int32), parent=dev(np.full(N_TAB, -1, np.int32)), kf_flags=dev(np.ones(N_TAB, np.uint8)))
        every = mappoint.covisibility_outputs(N_TAB, N_TAB, N_TAB, zeros)
        covisibility(list(range(N_TAB)), every)
        every["weight"][:, N_TAB - 1] = 0
        first = [(cn.UPDATE, k, k) for k in range(N_TAB - 1)]
        cn.apply_device(m, N_TAB, N_TAB, N_TAB, len(first), N_TAB, 0, TH, dict(weight=every["weight"], ops=dev(cn.pack_ops(first))), g,
                        cn.outputs(len(first), N_TAB, zeros))
        m.sync()
        entry = {k: v.clone() for k, v in g.items()}
        degree = float(entry["n_conn"][:N_TAB - 1].float().mean())

        # the log after a keyframe: the new keyframe and its best neighbour are updated, three keyframes are culled
        cur, near = N_TAB - 1, N_TAB - 3
        ops = [(cn.UPDATE, cur, 0), (cn.UPDATE, near, 1), (cn.KF_BAD, 150), (cn.KF_BAD, 100), (cn.KF_BAD, 50)]
        ins = dict(ops=dev(cn.pack_ops(ops)))
        rows = mappoint.covisibility_outputs(2, N_TAB, N_TAB, zeros)
        kfs = dev(np.array([cur, near], np.int32))
        out = cn.outputs(len(ops), N_TAB, zeros)
        for with_covisibility in (False, True):
            covisibility([cur, near], rows)
            times = []
            for rep in range(reps + 5):                                   # five warm-up calls
                for k in cn.INOUT_KEYS:
                    g[k].copy_(entry[k])
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(s)
                if with_covisibility:
                    mappoint.covisibility_device(m, N_TAB, CAP, N_PTS, 2, n_obs, N_TAB, TH, t["held_id"], t["n_kps"], t["pt_flags"], t["obs_off"],
                                                 t["obs_kf"], kfs, rows)
                cn.apply_device(m, N_TAB, N_TAB, 2, len(ops), N_TAB, 0, TH, dict(ins, weight=rows["weight"]), g, out)
                b.record(s)
                b.synchronize()
                if rep >= 5:
                    times.append(a.elapsed_time(b) * 1e3)
            counts, status = out["counts"].cpu().numpy(), out["op_status"].cpu().numpy()
            print(json.dumps(dict(what="msl_covisibility + msl_connections_apply" if with_covisibility else "msl_connections_apply", keyframes=N_TAB,
                                  ops=len(ops), mean_degree=round(degree, 1), op_status=status.tolist(), touched=int(counts[0]), turned_bad=int(counts[1]),
                                  change_parent=int(counts[2]), lib=lib, **percentiles(times))), flush=True)
    m.sync()
    m.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 30)

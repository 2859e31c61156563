"""Time Tracking::UpdateLocalMap on the device -- msl_local_keyframes, msl_local_points and msl_local_lines on device-resident tables -- at a
tracking-sized shape: 200 keyframes of 1000 keypoints and 100 keylines along a trajectory (keyframe k holds points 25 k .. 25 k + 999, so a
frame's points vote for about 80 keyframes), 5 975 map points, 1 090 map lines, batches of 1 and 64 frames.  Beside it the same stage by the
host path a caller uses today: download the tables, run a vectorised numpy form of tests/localmap_model.py per frame, upload the arrays the
matchers read.  The two results are compared before anything is timed.
Clock: the device steps as tools/rate_common.py (HIP events on the handle's stream around the three calls, median of five after a warm-up);
the host steps time.perf_counter around download + numpy + upload with the device idle before and after, median of five.  Every step runs in
a child process of its own under a time limit, and the steps stop at the first that fails.  Prints one JSON line per step.
Kernel times: `rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/localmap_rate.py --inline` (a run of its own,
all steps in one process; tracing slows the host, so the JSON lines of that run are not the rate)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.rate_common import main, time_calls, to_device as dev, zeros  # noqa: E402
STEPS = ("device1", "device64", "host1", "host64")
N_TAB, CAP, STEP, KLCAP, LSTEP, CCAP, MCAP, MLCAP = 200, 1000, 25, 100, 5, 30, 4096, 1024


def workload(n_frames, seed=1):
    """The arrays of msl.h for the trajectory map and n_frames frames spread along it, conn / n_conn left to msl_covisibility."""
    r = np.random.RandomState(seed)
    n_pts, n_lines = STEP * (N_TAB - 1) + CAP, LSTEP * (N_TAB - 1) + KLCAP
    held = (STEP * np.arange(N_TAB)[:, None] + np.arange(CAP)[None, :]).astype(np.int32)
    held[r.rand(N_TAB, CAP) < 0.1] = -1
    lheld = (LSTEP * np.arange(N_TAB)[:, None] + np.arange(KLCAP)[None, :]).astype(np.int32)
    obs = [[] for _ in range(n_pts)]
    for k in range(N_TAB):
        for p in held[k][held[k] >= 0]:
            obs[p].append(k)
    off = np.zeros(n_pts + 1, np.int32); off[1:] = np.cumsum([len(o) for o in obs])
    centre = np.linspace(50, 150, n_frames).astype(int) if n_frames > 1 else np.array([100])
    cur = (STEP * centre[:, None] + np.arange(CAP)[None, :]).astype(np.int32)
    cur[r.rand(n_frames, CAP) < 0.3] = -1
    cur_l = (LSTEP * centre[:, None] + np.arange(KLCAP)[None, :]).astype(np.int32)
    cur_l[r.rand(n_frames, KLCAP) < 0.5] = -1
    a = dict(held_id=held, n_kps=np.full(N_TAB, CAP, np.int32), kf_flags=(r.rand(N_TAB) > 0.03).astype(np.uint8), obs_off=off,
             obs_kf=np.concatenate(obs).astype(np.int32), parent=np.arange(-1, N_TAB - 1).astype(np.int32),
             pt_flags=(r.rand(n_pts) > 0.05).astype(np.uint8), pt_nobs=np.diff(off).astype(np.int32), pt_xyz=r.rand(n_pts, 3).astype(np.float32),
             pt_normal=r.rand(n_pts, 3).astype(np.float32), pt_dist=r.rand(n_pts, 2).astype(np.float32),
             pt_desc=r.randint(0, 256, (n_pts, 32)).astype(np.uint8), lheld_id=lheld, n_kl=np.full(N_TAB, KLCAP, np.int32),
             ln_flags=(r.rand(n_lines) > 0.05).astype(np.uint8), ln_nobs=r.randint(0, 5, n_lines).astype(np.int32), ln_xyz=r.rand(n_lines, 6),
             ln_normal=r.rand(n_lines, 3), ln_dist=r.rand(n_lines, 2).astype(np.float32), ln_desc=r.randint(0, 256, (n_lines, 32)).astype(np.uint8),
             cur_held=cur, n_cur=np.full(n_frames, CAP, np.int32), cur_lheld=cur_l, n_cur_lines=np.full(n_frames, KLCAP, np.int32))
    return a, dict(n_pts=n_pts, n_lines=n_lines, n_obs_total=int(off[-1]))


def host_frame(t, cur, cur_l):
    """UpdateLocalMap and the two first loops of one frame on host arrays, vectorised where the reference loops over elements.  Returns the
    arrays the matchers read (and local_kf, ref_kf)."""
    live = (cur >= 0) & (t["pt_flags"][np.maximum(cur, 0)] == 1)
    ids = cur[live]
    b, n = t["obs_off"][ids], t["obs_off"][ids + 1] - t["obs_off"][ids]
    idx = np.repeat(b - np.concatenate([[0], np.cumsum(n)[:-1]]), n) + np.arange(n.sum())
    votes = np.bincount(t["obs_kf"][idx], minlength=N_TAB)
    kf_live = (t["kf_flags"] & 1) != 0                                 # bit 0 alone: msl_connections_apply sets bit 2 as well
    first = np.nonzero((votes > 0) & kf_live)[0]
    local, mark = list(first), np.zeros(N_TAB, bool)
    mark[first] = True
    ref = int(first[np.argmax(votes[first])]) if len(first) else -1
    for k in first:
        if len(local) > 80:
            break
        for group in (t["conn"][k, :min(10, t["n_conn"][k], CCAP)], np.nonzero(t["parent"] == k)[0]):
            ok = group[kf_live[group] & ~mark[group]]
            if len(ok):
                local.append(int(ok[0])); mark[ok[0]] = True
        p = t["parent"][k]
        if p >= 0 and not mark[p]:
            local.append(int(p)); mark[p] = True
            break
    out = dict(local_kf=np.array(local, np.int32), ref_kf=ref)
    for pre, tab, held, mine, cap in (("mp", "pt", "held_id", cur, MCAP), ("ml", "ln", "lheld_id", cur_l, MLCAP)):
        flat = t[held][out["local_kf"]].reshape(-1)
        flat = flat[flat >= 0]
        flat = flat[t[tab + "_flags"][flat] == 1]
        _, at = np.unique(flat, return_index=True)
        loc = flat[np.sort(at)][:cap]
        mine_live = (mine >= 0) & (t[tab + "_flags"][np.maximum(mine, 0)] == 1)
        nobs = t[tab + "_nobs"]
        out[pre + "_id"] = loc
        out[pre + "_flags"] = (~np.isin(loc, mine[mine_live])).astype(np.uint8) | ((nobs[loc] > 0).astype(np.uint8) << 1)
        out[pre + "_cur_flags"] = np.where(mine_live, 1 | ((nobs[np.maximum(mine, 0)] > 0) << 1), 0).astype(np.uint8)
        for k in ("xyz", "normal", "dist", "desc"):
            out[pre + "_" + k] = t[tab + "_" + k][loc]
    return out


def run_step(step, a_):
    import torch
    from manhattanslam_amd import localmap, mappoint, match
    F = 64 if step.endswith("64") else 1
    a, sh = workload(F)
    m = match.Matcher()
    s = torch.cuda.Stream()
    m.set_stream(s.cuda_stream)
    d = {k: dev(v) for k, v in a.items()}
    covis = mappoint.covisibility_outputs(N_TAB, N_TAB, CCAP, zeros=zeros)
    with torch.cuda.stream(s):
        mappoint.covisibility_device(m, N_TAB, CAP, sh["n_pts"], N_TAB, sh["n_obs_total"], CCAP, 15, d["held_id"], d["n_kps"], d["pt_flags"], d["obs_off"],
                                     d["obs_kf"], dev(np.arange(N_TAB, dtype=np.int32)), covis)
    d["conn"], d["n_conn"] = covis["conn"], covis["n_conn"]
    kf = localmap.keyframes_outputs(F, CAP, N_TAB, zeros)
    pts, lns = localmap.points_outputs(F, CAP, MCAP, zeros), localmap.lines_outputs(F, KLCAP, MLCAP, zeros)
    d["local_kf"], d["n_local_kf"] = kf["local_kf"], kf["n_local_kf"]

    def device_call():
        localmap.local_keyframes_device(m, F, CAP, N_TAB, sh["n_pts"], sh["n_obs_total"], CCAP, d, kf)
        localmap.local_points_device(m, F, N_TAB, CAP, sh["n_pts"], MCAP, d, pts)
        localmap.local_lines_device(m, F, N_TAB, KLCAP, KLCAP, sh["n_lines"], MLCAP, d, lns)

    def host_call():
        t = {k: v.cpu().numpy() for k, v in d.items() if k not in ("local_kf", "n_local_kf")}     # the tables come down
        res = [host_frame(t, t["cur_held"][f], t["cur_lheld"][f]) for f in range(F)]
        up = [torch.from_numpy(np.ascontiguousarray(r[k])).cuda() for r in res for k in r if k not in ("local_kf", "ref_kf")]   # the matchers' arrays go up
        torch.cuda.synchronize()
        return res, up

    device_call(); m.sync()
    res, _ = host_call()
    n_kf, n_local = kf["n_local_kf"].cpu().numpy(), pts["n_local"].cpu().numpy()
    for f, r in enumerate(res):                                            # the two paths agree before either is timed
        assert np.array_equal(kf["local_kf"][f, :n_kf[f]].cpu().numpy(), r["local_kf"]) and int(kf["ref_kf"][f]) == r["ref_kf"]
        assert np.array_equal(pts["local_id"][f, :n_local[f]].cpu().numpy(), r["mp_id"]) and np.array_equal(pts["mp_flags"][f, :n_local[f]].cpu().numpy(), r["mp_flags"])
        assert np.array_equal(lns["ml_xyz"][f, :len(r["ml_id"])].cpu().numpy(), r["ml_xyz"]) and np.array_equal(pts["cur_flags"][f].cpu().numpy(), r["mp_cur_flags"])
    shape = dict(frames=F, keyframes=N_TAB, keypoints=CAP, local_keyframes=float(n_kf.mean()), local_points=float(n_local.mean()),
                 local_lines=float(lns["n_local_lines"].cpu().numpy().mean()))
    if step.startswith("device"):
        t = time_calls(s, device_call)
    else:
        times = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter(); host_call(); times.append((time.perf_counter() - t0) * 1e6)
        t = dict(us_per_call=round(float(np.median(times)), 2), us_calls=[round(x, 2) for x in times],
                 clock="time.perf_counter around download, numpy and upload, the device idle before and after; median of 5")
    print(json.dumps(dict(tool="localmap_rate", step=step, **shape, us_per_frame=round(t["us_per_call"] / F, 2), **t)), flush=True)
    m.close()


if __name__ == "__main__":
    main(__file__, STEPS, run_step, ())

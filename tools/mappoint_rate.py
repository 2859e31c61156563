"""Time msl_refresh_map_points and msl_covisibility on the device at the shape LocalMapping gives them: a 100-keyframe table of 1 000
keypoints per keyframe; one keyframe's 1 000 held points with 2 .. 30 observations each (most of them few: 2 + a geometric count, capped)
refreshed in one call, and its covisibility in one call; then the same for a batch of 32 keyframes (32 000 points, 32 counters).  Inputs and
outputs are device-resident (torch tensors); the refresh writes into the device point table.
Clock: HIP events on the handle's stream around one call; the median of five calls after a warm-up call.  Every step runs in a child
process of its own under a time limit, and the steps stop at the first that fails.  Prints one JSON line per step.
Kernel times: `rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/mappoint_rate.py --inline` (a run of its own,
all steps in one process; tracing slows the host, so the JSON lines of that run are not the rate)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.rate_common import main, time_calls, to_device as dev, zeros  # noqa: E402
STEPS = ("refresh_1", "covisibility_1", "refresh_32", "covisibility_32")


def workload(n_tab, n_kps, n_hold, max_obs, seed=1):
    """The first n_hold keyframes hold n_kps points each; a point is seen by its holder and by 1 .. max_obs - 1 other keyframes, each
    observation at a random keypoint.  Returns (table arrays, observation arrays, point arrays, held ids per holder)."""
    from manhattanslam_amd import KEYPOINT_DTYPE
    r = np.random.RandomState(seed)
    n_pts = n_hold * n_kps
    kps = np.zeros((n_tab, n_kps), KEYPOINT_DTYPE)
    kps["octave"] = r.randint(0, 8, (n_tab, n_kps))
    centres = np.stack([np.linspace(-2.0, 2.0, n_tab), 0.05 * np.sin(np.arange(n_tab)), 0.1 * np.cos(np.arange(n_tab))], 1)
    Tcw = np.stack([np.concatenate([np.eye(3), -c[:, None]], 1).reshape(12) for c in centres]).astype(np.float32)
    held = np.full((n_tab, n_kps), -1, np.int32)
    held[:n_hold] = np.arange(n_pts, dtype=np.int32).reshape(n_hold, n_kps)
    n_obs = np.minimum(2 + r.geometric(0.15, n_pts) - 1, max_obs)
    off = np.zeros(n_pts + 1, np.int32)
    off[1:] = np.cumsum(n_obs)
    okf = np.zeros(off[-1], np.int32); oidx = np.zeros(off[-1], np.int32)
    for p in range(n_pts):
        k = p // n_kps
        others = r.permutation(n_tab - 1)[:n_obs[p] - 1]
        kf = np.sort(np.concatenate([[k], others + (others >= k)]))                 # creation order
        okf[off[p]:off[p + 1]] = kf
        oidx[off[p]:off[p + 1]] = np.where(kf == k, p % n_kps, r.randint(0, n_kps, len(kf)))
    z = r.uniform(2.0, 8.0, n_pts)
    xyz = np.stack([r.uniform(-0.9, 0.9, n_pts) * z, r.uniform(-0.6, 0.6, n_pts) * z, z], 1).astype(np.float32)
    table = dict(kps_un=kps, desc=r.randint(0, 256, (n_tab, n_kps, 32)).astype(np.uint8), n_kps=np.full(n_tab, n_kps, np.int32), Tcw=Tcw,
                 kf_flags=np.ones(n_tab, np.uint8), held_id=held)
    obs = dict(obs_off=off, obs_kf=okf, obs_idx=oidx)
    points = dict(pt_xyz=xyz, pt_flags=np.ones(n_pts, np.uint8), pt_ref=(np.arange(n_pts) // n_kps).astype(np.int32))
    return table, obs, points, n_obs


def run_step(step, a):
    import torch
    from manhattanslam_amd import mappoint, match
    kind, n_kf = step.rsplit("_", 1)
    n_kf = int(n_kf)
    table, obs, points, n_obs = workload(a.n_tab, a.n_kps, 32, a.max_obs)
    d_t = {k: dev(v) for k, v in table.items()}; d_o = {k: dev(v) for k, v in obs.items()}; d_p = {k: dev(v) for k, v in points.items()}
    n_pts, total = len(points["pt_flags"]), int(obs["obs_off"][-1])
    m = match.Matcher()
    s = torch.cuda.Stream()
    m.set_stream(s.cuda_stream)
    sf = np.ones(8, np.float32)
    for i in range(1, 8):
        sf[i] = sf[i - 1] * np.float32(1.2)
    if kind == "refresh":
        n_items = n_kf * a.n_kps
        ids = dev(np.arange(n_items, dtype=np.int32))
        out = mappoint.refresh_outputs(n_items, zeros=zeros)
        rows = dict(pt_desc=zeros((n_pts, 32), np.uint8), pt_normal=zeros((n_pts, 3), np.float32), pt_dist=zeros((n_pts, 2), np.float32))
        prm = mappoint.refresh_params(sf)
        call = lambda: mappoint.refresh_map_points_device(m, prm, a.n_tab, a.n_kps, n_pts, n_items, total, 3, d_t, d_o, d_p, ids, out, rows)
        shape = dict(items=n_items, observations=int(n_obs[:n_items].sum()), obs_min=int(n_obs.min()), obs_median=float(np.median(n_obs)),
                     obs_max=int(n_obs.max()))
    else:
        kf = dev(np.arange(n_kf, dtype=np.int32))
        out = mappoint.covisibility_outputs(n_kf, a.n_tab, a.n_tab, zeros=zeros)
        call = lambda: mappoint.covisibility_device(m, a.n_tab, a.n_kps, n_pts, n_kf, total, a.n_tab, 15, d_t["held_id"], d_t["n_kps"], d_p["pt_flags"],
                                                    d_o["obs_off"], d_o["obs_kf"], kf, out)
        shape = dict(items=n_kf, observations_walked=int(n_obs[:n_kf * a.n_kps].sum()))
    line = dict(tool="mappoint_rate", step=step, n_tab=a.n_tab, n_kps=a.n_kps, **shape, **time_calls(s, call))
    if kind == "refresh":
        line["status_counts"] = np.bincount(out["status"].cpu().numpy(), minlength=4).tolist()
    else:
        line["n_conn"] = out["n_conn"].cpu().numpy()[:4].tolist()
    print(json.dumps(line), flush=True)
    m.close()


if __name__ == "__main__":
    main(__file__, STEPS, run_step, (("n-tab", 100), ("n-kps", 1000), ("max-obs", 30)))

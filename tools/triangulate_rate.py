"""Time msl_triangulate_new_points (LocalMapping::CreateNewMapPoints on the device) at the reference's shape -- 1 000 keypoints per keyframe,
10 neighbours per current keyframe, ~100 vocabulary nodes -- for 1 and 32 items per call over a table of 16 keyframes.  Inputs and outputs
are device-resident (torch tensors): one call = the five launches on the handle's stream.
Clock: the host's monotonic clock around `iters` calls that end in msl_match_sync, after warm-up calls of the same shape.  Prints one JSON
line per batch size.  Kernel times: run this under `rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python
tools/triangulate_rate.py` (a run of its own; tracing slows the host, so the JSON lines of that run are not the rate)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.rate_common import to_device  # noqa: E402


def workload(n_kf, n_kps, n_nodes, seed=1):
    """n_kf keyframes on an arc, every point seen by about 60 % of them, padded with clutter to n_kps keypoints each."""
    from tests import triangulate_scenes as ts
    r = np.random.RandomState(seed)
    poses = [ts.make_pose((0.15 * k, 0.03 * np.sin(k), 0.02 * np.cos(2 * k)), (0.0, -0.01 * k, 0.0)) for k in range(n_kf)]
    B = ts.Builder(seed + 1, poses)
    for X in ts._points(r, int(n_kps / 0.6), 2.0, 6.0, 0.5) + np.array([0.15 * n_kf / 2, 0, 0]):
        views = [k for k in range(n_kf) if r.uniform() < 0.6 and len(B.feats[k]) < n_kps]
        if len(views) >= 2:
            B.track(X, views, node=r.randint(n_nodes), held=[k for k in views if r.uniform() < 0.3])
    for k in range(n_kf):
        B.clutter(k, n_kps - len(B.feats[k]), node_range=(0, n_nodes))
    return B.finish()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", default="1,32")
    ap.add_argument("--n-kps", type=int, default=1000)
    ap.add_argument("--neighbours", type=int, default=10)
    ap.add_argument("--keyframes", type=int, default=16)
    ap.add_argument("--nodes", type=int, default=100)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    import torch
    from manhattanslam_amd import match, triangulate
    from tests import triangulate_scenes as ts
    table = workload(a.keyframes, a.n_kps, a.nodes)
    mp = ts.prm()
    prm = triangulate.triangulate_params(ts.FX, ts.FY, ts.CX, ts.CY, ts.BF, mp["scale_factors"], mp["level_sigma2"], 1.2)
    cap, t = triangulate.pack_table(table)
    d_t = {k: to_device(v) for k, v in t.items()}
    m = match.Matcher()
    tdt = {np.dtype(np.int32): torch.int32, np.dtype(np.uint8): torch.uint8, np.dtype(np.float32): torch.float32}
    for F in (int(x) for x in a.items.split(",")):
        items = [(f % a.keyframes, [(f + 1 + q) % a.keyframes for q in range(a.neighbours)]) for f in range(F)]
        ncap, cur, neigh, n_neigh = triangulate.pack_items(items)
        d_i = [torch.from_numpy(x).cuda() for x in (cur, neigh, n_neigh)]
        out = triangulate.outputs(F, ncap, cap, zeros=lambda shape, dt: torch.empty(shape, dtype=tdt[np.dtype(dt)], device="cuda"))
        torch.cuda.synchronize()
        run = lambda: triangulate.triangulate_new_points_device(m, prm, len(table), cap, F, ncap, d_t, *d_i, out)
        for _ in range(a.warmup):
            run()
        m.sync()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            run()
        m.sync()
        dt = time.perf_counter() - t0
        print(json.dumps({"tool": "triangulate_rate", "items_per_call": F, "n_kps": a.n_kps, "neighbours": a.neighbours, "keyframes": a.keyframes,
                          "nodes": a.nodes, "iters": a.iters, "us_per_call": round(dt / a.iters * 1e6, 2), "us_per_item": round(dt / a.iters / F * 1e6, 3),
                          "nmatches_mean_per_pair": float(out["nmatches"].float().mean()), "n_new_mean": float(out["n_new"].float().mean()),
                          "clock": "host perf_counter around iters calls ending in msl_match_sync"}), flush=True)
    m.close()


if __name__ == "__main__":
    main()

"""Time msl_match_local_points (Tracking::SearchLocalPoints on the device) at 1 000 keypoints x 4 000 local map points per frame, for 1 and
32 frames per call.  Inputs and outputs are device-resident (torch tensors): one call = the four launches on the handle's stream.
Clock: the host's monotonic clock around `iters` calls that end in msl_match_sync, after warm-up calls of the same shape.  Prints one JSON
line per batch size.  Kernel times: run this under `rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/local_match_rate.py` (a run of
its own; tracing slows the host, so the JSON lines of that run are not the rate)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="1,32")
    ap.add_argument("--n-cur", type=int, default=1000)
    ap.add_argument("--n-local", type=int, default=4000)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    import torch
    from manhattanslam_amd import KEYPOINT_DTYPE, LOCAL_TRACK_DTYPE, match
    from tests import local_match_scenes as ls
    p = ls.params(3.0)
    m = match.Matcher()
    for B in (int(x) for x in a.frames.split(",")):
        frames = [ls.random_frame(1000 + f, p, n_cur=a.n_cur, n_local=a.n_local) for f in range(B)]
        cap, mcap, arrays = match.pack_local_points([f[0] for f in frames], [f[1] for f in frames], np.stack([f[2] for f in frames]))
        dev = [torch.from_numpy(np.ascontiguousarray(x.view(np.uint8) if x.dtype == KEYPOINT_DTYPE else x)).cuda() for x in arrays]
        mo = torch.empty((B, cap), dtype=torch.int32, device="cuda"); ntm = torch.empty(B, dtype=torch.int32, device="cuda")
        nm = torch.empty(B, dtype=torch.int32, device="cuda"); inv = torch.empty((B, mcap), dtype=torch.uint8, device="cuda")
        trk = torch.empty((B, mcap * LOCAL_TRACK_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for _ in range(a.warmup):
            m.search_local_points_device(p, B, cap, mcap, dev, mo, ntm, nm, inv, trk)
        m.sync()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            m.search_local_points_device(p, B, cap, mcap, dev, mo, ntm, nm, inv, trk)
        m.sync()
        dt = time.perf_counter() - t0
        print(json.dumps({"tool": "local_match_rate", "frames_per_call": B, "n_cur": a.n_cur, "n_local": a.n_local, "iters": a.iters,
                          "us_per_call": round(dt / a.iters * 1e6, 2), "us_per_frame": round(dt / a.iters / B * 1e6, 3),
                          "n_to_match_mean": float(ntm.float().mean()), "nmatches_mean": float(nm.float().mean()),
                          "clock": "host perf_counter around iters calls ending in msl_match_sync"}), flush=True)
    m.close()


if __name__ == "__main__":
    main()

"""Time msl_pose_optimize_translation (Optimizer::TranslationOptimization on the device, Manhattan mode) at 1 000 points + 40 lines + 6 planes
per frame (only the mvpMapPlanes kind is read), with a Manhattan rotation Rcw per frame, for 1, 32 and 256 frames per call.  The shape and
the clock are tools/pose_opt_rate.py's, so the two rates compare directly.  Inputs and outputs are device-resident (torch tensors): one
call = one launch on the matcher handle's stream.  The outlier flags are restored from a device copy before every call (a device-to-device copy on the same
stream, inside the timed loop), so every call optimises the same problem.  Clock: the host's monotonic clock around `iters` calls that end
in msl_match_sync, after warm-up calls of the same shape.  Prints one JSON line per batch size.  Kernel times: run this under
`rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/translation_opt_rate.py` (a run of its own; tracing slows the host,
so the JSON lines of that run are not the rate).  There is no g2o baseline here: only GPU times are reported."""
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
    ap.add_argument("--frames", default="1,32,256")
    ap.add_argument("--n-pts", type=int, default=1000)
    ap.add_argument("--n-lines", type=int, default=40)
    ap.add_argument("--n-planes", type=int, default=6)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    from manhattanslam_amd import KEYPOINT_DTYPE, pose
    from manhattanslam_amd.match import Matcher
    from tests import pose_scenes as ps
    from tests import translation_scenes as ts
    c = ps.params()
    p = pose.pose_params(c)
    m = Matcher()
    base = [ts.scene(2000 + f, n_pts=a.n_pts, n_lines=a.n_lines, n_planes=a.n_planes, margin=None)[:2] for f in range(32)]
    for B in (int(x) for x in a.frames.split(",")):
        frames = [base[f % len(base)][0] for f in range(B)]
        rcw = torch.from_numpy(np.stack([base[f % len(base)][1] for f in range(B)])).cuda()
        caps, arrays, io = pose.pack(frames)
        dev = [torch.from_numpy(np.ascontiguousarray(x.view(np.uint8) if x.dtype == KEYPOINT_DTYPE else x)).cuda() for x in arrays]
        io0 = [torch.from_numpy(x).cuda() for x in io]
        iod = [x.clone() for x in io0]
        Tout = torch.zeros((B, 12), dtype=torch.float32, device="cuda"); ng = torch.zeros(B, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def call():
            for x, y in zip(iod, io0):
                x.copy_(y)
            pose.translation_optimization_device(m, p, B, caps, dev, iod, Tout, ng, rcw=rcw)

        for _ in range(a.warmup):
            call()
            torch.cuda.synchronize(); m.sync()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            call()
            torch.cuda.synchronize(); m.sync()
        dt = time.perf_counter() - t0
        print(json.dumps({"tool": "translation_opt_rate", "frames_per_call": B, "n_pts": a.n_pts, "n_lines": a.n_lines, "n_planes": a.n_planes,
                          "iters": a.iters, "us_per_call": round(dt / a.iters * 1e6, 2), "us_per_frame": round(dt / a.iters / B * 1e6, 3),
                          "n_good_mean": float(ng.float().mean()),
                          "clock": "host perf_counter around iters calls (flag reset + launch) ending in msl_match_sync"}), flush=True)
    m.close()


if __name__ == "__main__":
    main()

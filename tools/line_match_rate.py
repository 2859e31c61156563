"""Time the two map-line searches on the device: msl_match_lines_by_projection (40 keylines x 40 last-frame lines) and msl_match_local_lines
(40 keylines x 2 000 local map lines), for 1 and 32 frames per call.  Inputs and outputs are device-resident (torch tensors), line_xyz /
line_has included: one call = the two launches on the handle's stream.  Clock: the host's monotonic clock around `iters` calls that end in
msl_match_sync, after warm-up calls of the same shape.  Prints one JSON line per (search, batch size).  Kernel times: run this under
`rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/line_match_rate.py` (a run of its own; tracing slows the host,
so the JSON lines of that run are not the rate)."""
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
    ap.add_argument("--n-kl", type=int, default=40)
    ap.add_argument("--n-last", type=int, default=40)
    ap.add_argument("--n-local", type=int, default=2000)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    import torch
    from manhattanslam_amd import KEYLINE_DTYPE, LINE_TRACK_DTYPE, match
    from tests import line_match_scenes as lsc
    pl, plo = lsc.params(15.0), lsc.params(1.0)
    m = match.Matcher()
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x.view(np.uint8) if x.dtype == KEYLINE_DTYPE else x)).cuda()

    def timed(call):
        for _ in range(a.warmup):
            call()
        m.sync()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            call()
        m.sync()
        return time.perf_counter() - t0

    for B in (int(x) for x in a.frames.split(",")):
        pairs = [lsc.frame_pair(2000 + f, pl, n_kl=a.n_kl, n_last=a.n_last) for f in range(B)]
        lcap, llcap, arrays = match.pack_lines_last([q[0] for q in pairs], [q[1] for q in pairs], np.stack([q[2] for q in pairs]),
                                                    np.stack([q[3] for q in pairs]))
        d = [dev(x) for x in arrays]
        mo = torch.empty((B, lcap), dtype=torch.int32, device="cuda"); nm = torch.empty(B, dtype=torch.int32, device="cuda")
        lx = torch.zeros((B, lcap, 6), dtype=torch.float64, device="cuda"); lh = torch.zeros((B, lcap), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        dt = timed(lambda: m.search_lines_by_projection_device(pl, B, lcap, llcap, d, mo, nm, lx, lh))
        print(json.dumps({"tool": "line_match_rate", "search": "last_frame", "frames_per_call": B, "n_kl": a.n_kl, "n_lines": a.n_last,
                          "iters": a.iters, "us_per_call": round(dt / a.iters * 1e6, 2), "us_per_frame": round(dt / a.iters / B * 1e6, 3),
                          "nmatches_mean": float(nm.float().mean()), "clock": "host perf_counter around iters calls ending in msl_match_sync"}),
              flush=True)

        frames = [lsc.local_frame(3000 + f, plo, n_kl=a.n_kl, n_local=a.n_local) for f in range(B)]
        lcap, mlcap, arrays = match.pack_local_lines([q[0] for q in frames], [q[1] for q in frames], np.stack([q[2] for q in frames]))
        d = [dev(x) for x in arrays]
        mo = torch.empty((B, lcap), dtype=torch.int32, device="cuda"); nm = torch.empty(B, dtype=torch.int32, device="cuda")
        ntm = torch.empty(B, dtype=torch.int32, device="cuda"); inv = torch.empty((B, mlcap), dtype=torch.uint8, device="cuda")
        trk = torch.empty((B, mlcap * LINE_TRACK_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
        lx = torch.zeros((B, lcap, 6), dtype=torch.float64, device="cuda"); lh = torch.zeros((B, lcap), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        dt = timed(lambda: m.search_local_lines_device(plo, B, lcap, mlcap, d, mo, ntm, nm, inv, trk, lx, lh))
        print(json.dumps({"tool": "line_match_rate", "search": "local_map", "frames_per_call": B, "n_kl": a.n_kl, "n_lines": a.n_local,
                          "iters": a.iters, "us_per_call": round(dt / a.iters * 1e6, 2), "us_per_frame": round(dt / a.iters / B * 1e6, 3),
                          "n_to_match_mean": float(ntm.float().mean()), "nmatches_mean": float(nm.float().mean()),
                          "clock": "host perf_counter around iters calls ending in msl_match_sync"}), flush=True)
    m.close()


if __name__ == "__main__":
    main()

"""Latency of msl_plane_clouds and msl_map_plane_merge in device memory on one matcher handle, by event pairs on the handle's stream (the
method of tools/peac_latency.py's device-resident call): one frame of 8 planes over 76 800 vertices, a batch of 32 such frames, and the
merge of a frame's 8 plane clouds into a map of 64 rows (one frame and 32).  One JSON line per measurement: the median, minimum and 90th
percentile of `reps` calls in microseconds.  MSL_LIB selects a variant library (tools/build_variant.sh) for an ablation."""
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from manhattanslam_amd import plane_cloud
from manhattanslam_amd.match import Matcher

W, H, PLANES, ROWS = 320, 240, 8, 64


def frame(seed):
    """An organised 320 x 240 cloud of 8 vertical strips, each a wall of its own about 3 m x 2.4 m at 2 to 4 m."""
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    cloud = np.zeros((H, W, 3))
    planes, vertices = [], []
    for p in range(PLANES):
        sel = (u // (W // PLANES)) == p
        n = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), 1.0]); n /= np.linalg.norm(n)
        z0 = rng.uniform(2.0, 4.0)
        x = (u[sel] % (W // PLANES)) / (W // PLANES) * 3.0 - 1.5 + 4.0 * p
        y = v[sel] / H * 2.4 - 1.2
        z = z0 - (n[0] * (x - 4.0 * p) + n[1] * y) / n[2] + rng.normal(0, 0.003, x.shape)
        cloud[sel] = np.stack([x, y, z], axis=1)
        planes.append((n, np.array([4.0 * p, 0.0, z0])))
        vertices.append(np.flatnonzero(sel.reshape(-1)).astype(np.int32))
    rgb = rng.integers(0, 256, (H * W, 3)).astype(np.uint8)
    return dict(cloud=cloud.reshape(-1, 3), rgb=rgb, vertices=vertices, planes=planes, seed=seed)


def dev(a):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype.fields is not None or a.dtype == np.uint32:
        a = a.view(np.uint8)
    return torch.from_numpy(a).cuda()


def timed(stream, fn, reps):
    for _ in range(5):
        fn()
    stream.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    out.sort()
    return dict(med_us=round(out[len(out) // 2], 1), min_us=round(out[0], 1), p90_us=round(out[int(len(out) * 0.9)], 1))


def main(reps=50):
    prm = plane_cloud.plane_cloud_params()
    s = torch.cuda.Stream()
    m = Matcher()
    m.set_stream(s.cuda_stream)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    pcap, ptcap = PLANES, PLANES * 1024
    for F in (1, 32):
        frames = [frame(100 + f) for f in range(F)]
        V, P, _, arrays = plane_cloud.pack_clouds(frames)
        with torch.cuda.stream(s):
            d = [dev(a) for a in arrays]
            outs = [z((F,), torch.int32), z((F, pcap, 4), torch.float32), z((F, pcap), torch.int32), z((F, pcap), torch.int32),
                    z((F, pcap + 1), torch.int32), z((F, ptcap, 3), torch.float32), z((F, ptcap, 3), torch.uint8), z((F, P), torch.int32)]
            r = timed(s, lambda: plane_cloud.plane_clouds_device(m, prm, F, V, P, pcap, ptcap, d, *outs), reps)
            print(json.dumps(dict(what="msl_plane_clouds", frames=F, planes=PLANES, vertices=V, kept=int(outs[0].sum()),
                                  coarse_points=int(outs[2].sum()), lib=os.environ.get("MSL_LIB", "product"), **r)), flush=True)
            # the merge: the frame's clouds into the first 8 of 64 map rows, every row about 300 points
            rng = np.random.default_rng(7)
            mcap, mptcap = ROWS, ROWS * 512
            moff = np.zeros((F, mcap + 1), np.int32); mpts = np.zeros((F, mptcap, 3), np.float32); mrgb = np.zeros((F, mptcap, 3), np.uint8)
            for f in range(F):
                o = 0
                for j in range(ROWS):
                    c = np.stack([rng.uniform(-1.5, 1.5, 300) + 4.0 * (j % PLANES), rng.uniform(-1.2, 1.2, 300), rng.uniform(2.0, 4.0) + rng.normal(0, 0.01, 300)], axis=1)
                    mpts[f, o:o + 300] = c; o += 300; moff[f, j + 1] = o
            into = np.tile(np.arange(PLANES, dtype=np.int32), (F, 1))
            Twc = np.tile(np.array([1, 0, 0, 0.05, 0, 1, 0, -0.02, 0, 0, 1, 0.03], np.float64), (F, 1))
            marr = [outs[0], outs[4], outs[5], outs[6], dev(into), dev(Twc), dev(moff), dev(mpts), dev(mrgb), dev(np.full(F, ROWS, np.int32))]
            mo = [z((F, mcap + 1), torch.int32), z((F, mptcap, 3), torch.float32), z((F, mptcap, 3), torch.uint8), z((F, mcap), torch.int32)]
            r = timed(s, lambda: plane_cloud.map_plane_merge_device(m, prm, F, (pcap, ptcap, mcap, mptcap), marr, *mo), reps)
            print(json.dumps(dict(what="msl_map_plane_merge", frames=F, rows=ROWS, merged=int((mo[3] == 1).sum()), map_points=int(mo[0][:, -1].sum()),
                                  lib=os.environ.get("MSL_LIB", "product"), **r)), flush=True)
    m.sync()
    m.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 50)

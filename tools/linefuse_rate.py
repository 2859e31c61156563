"""Time the line half of LocalMapping::SearchInNeighbors on the device: msl_fuse_map_lines with 40 items sharing one 40-line list at 40
keylines per keyframe (the reference's own sizes: the current keyframe's lines into every target), msl_fuse_map_lines with one item of
25 000 candidates at 256 keylines (the ABI's keyframe limit; the candidates are shifted copies of 256 segments, about 98 per keyline), and
msl_refresh_map_lines for 1 000 lines of 8 observations.  Inputs and outputs are device-resident (torch tensors).
Clock: HIP events on the handle's stream around one call; the median of five calls after a warm-up call.  Every step runs in a child
process of its own under a time limit, and the steps stop at the first that fails.  Prints one JSON line per step.
Kernel times: `rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/linefuse_rate.py --inline` (a run of its own,
all steps in one process; tracing slows the host, so the JSON lines of that run are not the rate)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.rate_common import main, time_calls, to_device as dev, zeros  # noqa: E402
STEPS = ("targets", "current", "refresh")
FX = FY = 517.3; CX, CY, W, H = 318.6, 255.3, 640.0, 480.0


def workload(n_kf, n_kl, n_lines, seed=1):
    """n_kf keyframes side by side in front of a wall of n_kl segments, each with a keyline on every segment (pixel noise, the octave its
    distance predicts, a noisy copy of the segment's descriptor); n_lines map lines, line i a slightly shifted copy of segment i % n_kl;
    keyframe 0 holds the first n_kl of them, the others hold every second one.  Returns (table, lines, observations)."""
    from manhattanslam_amd import KEYLINE_DTYPE
    r = np.random.RandomState(seed)
    sf = 1.2 ** np.arange(8)
    centres = np.stack([np.linspace(-0.5, 0.5, n_kf), 0.05 * np.sin(np.arange(n_kf)), 0.1 * np.cos(np.arange(n_kf))], 1)
    centres[0] = 0.0
    z = r.uniform(3.0, 6.0, n_kl)
    a = np.stack([r.uniform(-0.35, 0.35, n_kl) * z, r.uniform(-0.3, 0.3, n_kl) * z, z], 1)
    d = r.normal(0, 1, (n_kl, 3)); d[:, 2] *= 0.2
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * r.uniform(0.2, 0.5, (n_kl, 1))
    seg = np.concatenate([a - 0.5 * d, a + 0.5 * d], 1)
    D = np.linalg.norm(a, axis=1) * 1.2 ** r.randint(0, 5, n_kl) * r.uniform(1.02, 1.15, n_kl)
    desc = r.randint(0, 256, (n_kl, 32)).astype(np.uint8)
    table = []
    for k in range(n_kf):
        P1, P2 = seg[:, :3] - centres[k], seg[:, 3:] - centres[k]
        u1 = FX * P1[:, 0] / P1[:, 2] + CX; v1 = FY * P1[:, 1] / P1[:, 2] + CY
        u2 = FX * P2[:, 0] / P2[:, 2] + CX; v2 = FY * P2[:, 1] / P2[:, 2] + CY
        kl = np.zeros(n_kl, KEYLINE_DTYPE)
        kl["x"] = 0.5 * (u1 + u2) + r.normal(0, 0.4, n_kl); kl["y"] = 0.5 * (v1 + v2) + r.normal(0, 0.4, n_kl)
        kl["angle"] = (v1 - v2) / (u1 - u2) + r.uniform(0.02, 0.3, n_kl)
        kl["octave"] = np.clip(np.ceil(np.log(D / np.linalg.norm(a - centres[k], axis=1)) / np.log(1.2)), 0, 7)
        noisy = desc.copy()
        flip = r.randint(0, 256, (n_kl, 6))
        for i in range(n_kl):
            for b in flip[i]:
                noisy[i, b >> 3] ^= 1 << (b & 7)
        held = np.arange(n_kl, dtype=np.int32)
        if k:
            held[1::2] = -1
        table.append(dict(kl=kl, ldesc=noisy, Tcw=np.concatenate([np.eye(3), -centres[k][:, None]], 1).astype(np.float32), held_id=held))
    src = np.arange(n_lines) % n_kl
    xyz = seg[src] + np.tile(r.normal(0, 0.003, (n_lines, 3)), 2) * (np.arange(n_lines) >= n_kl)[:, None]
    mid = 0.5 * (xyz[:, :3] + xyz[:, 3:])
    dist = np.linalg.norm(mid, axis=1)
    dmax = dist * sf[np.clip(np.ceil(np.log(D[src] / dist) / np.log(1.2)), 0, 7).astype(int)] * 0.96
    lines = dict(xyz=xyz, normal=mid / dist[:, None], dist=np.stack([dmax / sf[7], dmax], 1).astype(np.float32), desc=desc[src],
                 flags=np.ones(n_lines, np.uint8), nobs=r.randint(1, 9, n_lines).astype(np.int32), ref=np.zeros(n_lines, np.int32))
    obs = [[(int(k), int(src[i])) for k in range(min(n_kf, 8))] for i in range(n_lines)]
    return table, lines, obs


def run_step(step, a):
    import torch
    from manhattanslam_amd import linefuse, mappoint, match
    from manhattanslam_amd.fuse import pack_lists
    sf = np.ones(8, np.float32)
    for i in range(1, 8):
        sf[i] = sf[i - 1] * np.float32(1.2)
    prm = linefuse.line_fuse_params(FX, FY, CX, CY, 0.0, W, 0.0, H, sf, np.float32(np.log(1.2)))
    m = match.Matcher()
    s = torch.cuda.Stream()
    m.set_stream(s.cuda_stream)
    out = None
    if step == "targets":
        T = a.targets
        table, lines, _ = workload(T + 1, a.n_kl, a.n_kl)
        klcap, t = linefuse.pack_line_table(table)
        n_lines, p = linefuse.pack_lines(lines)
        d_t = {k: dev(v) for k, v in t.items()}; d_p = {k: dev(v) for k, v in p.items()}
        lcap, own, n_own = pack_lists([list(range(a.n_kl))])
        d_own, d_n = dev(own), dev(n_own)
        tgt, lst = dev(np.arange(1, T + 1, dtype=np.int32)), dev(np.zeros(T, np.int32))
        out = linefuse.outputs(T, lcap, zeros=zeros)
        call = lambda: linefuse.fuse_map_lines_device(m, prm, T + 1, klcap, n_lines, T, 1, lcap, d_t, d_p, tgt, lst, d_own, d_n, out)
        shape = dict(items=T, candidates_per_item=a.n_kl, keylines=a.n_kl)
    elif step == "current":
        table, lines, _ = workload(2, 256, a.candidates)
        klcap, t = linefuse.pack_line_table(table)
        n_lines, p = linefuse.pack_lines(lines)
        d_t = {k: dev(v) for k, v in t.items()}; d_p = {k: dev(v) for k, v in p.items()}
        lcap, cand, n_cand = pack_lists([list(range(a.candidates))])
        d_c, d_n = dev(cand), dev(n_cand)
        tgt, lst = dev(np.zeros(1, np.int32)), dev(np.zeros(1, np.int32))
        out = linefuse.outputs(1, lcap, zeros=zeros)
        call = lambda: linefuse.fuse_map_lines_device(m, prm, 2, klcap, n_lines, 1, 1, lcap, d_t, d_p, tgt, lst, d_c, d_n, out)
        shape = dict(items=1, candidates_per_item=a.candidates, keylines=256)
    else:
        table, lines, obs = workload(8, a.n_kl, a.refresh)
        klcap, t = linefuse.pack_line_table(table)
        n_lines, p = linefuse.pack_lines(lines)
        o = mappoint.pack_observations(obs)
        d_t = {k: dev(v) for k, v in t.items()}; d_p = {k: dev(v) for k, v in p.items()}; d_o = {k: dev(v) for k, v in o.items()}
        ids = dev(np.arange(a.refresh, dtype=np.int32))
        res = linefuse.refresh_outputs(a.refresh, zeros=zeros)
        rp = mappoint.refresh_params(sf)
        call = lambda: linefuse.refresh_map_lines_device(m, rp, 8, klcap, n_lines, a.refresh, int(o["obs_off"][-1]), d_t, d_o, d_p, ids, res, d_p)
        shape = dict(lines=a.refresh, observations_per_line=8)
    line = dict(tool="linefuse_rate", step=step, **shape, **time_calls(s, call))
    if out is not None:
        line["n_fused"] = int(out["n_fused"].sum())
        line["status_counts"] = np.bincount(out["status"].cpu().numpy().reshape(-1), minlength=15).tolist()
    else:
        line["written"] = int((res["status"].cpu().numpy() == 2).sum())
    print(json.dumps(line), flush=True)
    m.close()


if __name__ == "__main__":
    main(__file__, STEPS, run_step, (("n-kl", 40), ("targets", 40), ("candidates", 25000), ("refresh", 1000)))

"""Time the point half of LocalMapping::SearchInNeighbors on the device at the reference's shape -- 1 000 keypoints per keyframe, 40 target
keyframes: msl_fuse_map_points with 40 items sharing one 600-point list (the current keyframe's points into every target), then
msl_fuse_candidates over the 40 targets, then msl_fuse_map_points with one item of 25 000 candidates (the targets' points, filled up with
points no target holds, into the current keyframe).  Inputs and outputs are device-resident (torch tensors).
Clock: HIP events on the handle's stream around one call; the median of five calls after a warm-up call.  Every step runs in a child
process of its own under a time limit, and the steps stop at the first that fails.  Prints one JSON line per step.
Kernel times: `rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/fuse_rate.py --inline` (a run of its own, all
steps in one process; tracing slows the host, so the JSON lines of that run are not the rate)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.rate_common import main, time_calls, to_device as dev, zeros  # noqa: E402
STEPS = ("targets", "candidates", "current")
FX = FY = 517.3; CX, CY, BF, W, H = 318.6, 255.3, 40.0, 640.0, 480.0


def workload(n_kf, n_kps, n_list, seed=1):
    """n_kf keyframes side by side in front of a wall of points; every keyframe takes n_kps of the points it sees as keypoints (40 % by a
    priority all keyframes share, so neighbours see the same points; pixel noise, the octave its distance predicts) and holds the point of every keypoint, keyframe 0 only n_list of them.  Returns (table, points) as
    manhattanslam_amd.fuse packs them."""
    from manhattanslam_amd import KEYPOINT_DTYPE
    r = np.random.RandomState(seed)
    sf = 1.2 ** np.arange(8)
    centres = np.stack([np.linspace(-1.0, 1.0, n_kf), 0.05 * np.sin(np.arange(n_kf)), 0.1 * np.cos(np.arange(n_kf))], 1)
    centres[0] = 0.0
    n_w = 4 * n_kf * n_kps
    z = r.uniform(2.0, 8.0, n_w)
    X = np.stack([r.uniform(-0.9, 0.9, n_w) * z, r.uniform(-0.6, 0.6, n_w) * z, z], 1)
    D = z * 1.2 ** r.randint(0, 5, n_w) * r.uniform(1.02, 1.15, n_w)
    desc = r.randint(0, 256, (n_w, 32)).astype(np.uint8)
    prio = r.permutation(n_w)
    table = []
    for k in range(n_kf):
        Xc = X - centres[k]
        u = FX * Xc[:, 0] / Xc[:, 2] + CX; v = FY * Xc[:, 1] / Xc[:, 2] + CY
        vis = np.flatnonzero((u >= 1) & (u < W - 1) & (v >= 1) & (v < H - 1))
        shared = vis[np.argsort(prio[vis], kind="stable")[:int(0.4 * n_kps)]]      # what its neighbours see too ...
        rest = np.setdiff1d(vis, shared)
        pick = np.concatenate([shared, rest[r.permutation(len(rest))[:n_kps - len(shared)]]])   # ... and points of its own
        d = np.linalg.norm(Xc[pick], axis=1)
        kp = np.zeros(len(pick), KEYPOINT_DTYPE)
        kp["x"] = u[pick] + r.normal(0, 0.4, len(pick)); kp["y"] = v[pick] + r.normal(0, 0.4, len(pick))
        kp["octave"] = np.clip(np.ceil(np.log(D[pick] / d) / np.log(1.2)), 0, 7)
        px = np.round(kp["x"] * np.float32(64 / W)).astype(int); py = np.round(kp["y"] * np.float32(48 / H)).astype(int)
        stereo = r.uniform(size=len(pick)) < 0.5
        held = pick.astype(np.int32)
        if k == 0:
            held[n_list:] = -1
        else:                                                                  # 30 % empty slots, 30 % a duplicate of the point (id + n_w)
            what = r.uniform(size=len(pick))
            held = np.where(what < 0.3, -1, np.where(what < 0.6, held + n_w, held)).astype(np.int32)
        table.append(dict(kps_un=kp, uright=np.where(stereo, kp["x"] - BF / Xc[pick, 2], -1).astype(np.float32),
                          grid_cell=np.where((px >= 0) & (px < 64) & (py >= 0) & (py < 48), px * 48 + py, -1).astype(np.int32), desc=desc[pick],
                          Tcw=np.concatenate([np.eye(3), -centres[k][:, None]], 1).astype(np.float32), held_id=held))
    n = X / np.linalg.norm(X, axis=1, keepdims=True)
    dmax = np.linalg.norm(X, axis=1) * sf[np.clip(np.ceil(np.log(D / np.linalg.norm(X, axis=1)) / np.log(1.2)), 0, 7).astype(int)]
    two = lambda v: np.concatenate([v, v])                                     # every point and its duplicate
    points = dict(xyz=two(X.astype(np.float32)), normal=two(n.astype(np.float32)), dist=two(np.stack([dmax / sf[7], dmax], 1).astype(np.float32)),
                  desc=two(desc), flags=np.ones(2 * n_w, np.uint8), nobs=r.randint(2, 9, 2 * n_w).astype(np.int32))
    return table, points


def run_step(step, a):
    import torch
    from manhattanslam_amd import fuse, match
    table, points = workload(a.targets + 1, a.n_kps, a.list)
    sf = np.ones(8, np.float32)
    for i in range(1, 8):
        sf[i] = sf[i - 1] * np.float32(1.2)
    prm = fuse.fuse_params(FX, FY, CX, CY, BF, 0.0, W, 0.0, H, sf, np.float32(1.0) / (sf * sf), np.float32(np.log(1.2)))
    cap, t = fuse.pack_table(table)
    n_pts, p = fuse.pack_points(points)
    d_t = {k: dev(v) for k, v in t.items()}; d_p = {k: dev(v) for k, v in p.items()}
    m = match.Matcher()
    s = torch.cuda.Stream()
    m.set_stream(s.cuda_stream)
    T = a.targets
    targets = dev(np.arange(1, T + 1, dtype=np.int32)[None]); n_targets = dev(np.array([T], np.int32))
    cand = zeros((1, a.candidates), np.int32); n_cand = zeros((1,), np.int32)
    with torch.cuda.stream(s):
        fuse.fuse_candidates_device(m, T + 1, cap, n_pts, 1, T, a.candidates, d_t["held_id"], d_t["n_kps"], d_p["pt_flags"], targets, n_targets, cand, n_cand)
        n_cand.clamp_(max=a.candidates)
        n_again = zeros((1,), np.int32)
    s.synchronize()
    # the targets hold fewer distinct points than the reference's 25 000: the list is filled up with points no target holds
    have = cand[0, :int(n_cand[0])].cpu().numpy()
    fill = np.setdiff1d(np.arange(n_pts // 2, dtype=np.int32), have % (n_pts // 2))[:a.candidates - len(have)]
    from_targets = len(have)
    cand[0, :len(have) + len(fill)] = dev(np.concatenate([have, fill]).astype(np.int32))
    n_cand.fill_(len(have) + len(fill))
    torch.cuda.synchronize()
    if step == "targets":
        lcap, own, n_own = fuse.pack_lists([table[0]["held_id"][:a.list].tolist()])
        d_own, d_n = dev(own), dev(n_own)
        tgt, lst = dev(np.arange(1, T + 1, dtype=np.int32)), dev(np.zeros(T, np.int32))
        out = fuse.outputs(T, lcap, zeros=zeros)
        call = lambda: fuse.fuse_map_points_device(m, prm, T + 1, cap, n_pts, T, 1, lcap, d_t, d_p, tgt, lst, d_own, d_n, out)
        shape = dict(items=T, candidates_per_item=int(n_own[0]))
    elif step == "candidates":
        call = lambda: fuse.fuse_candidates_device(m, T + 1, cap, n_pts, 1, T, a.candidates, d_t["held_id"], d_t["n_kps"], d_p["pt_flags"], targets,
                                                   n_targets, cand, n_again)
        out = None
        shape = dict(items=1, targets=T)
    else:
        tgt, lst = dev(np.zeros(1, np.int32)), dev(np.zeros(1, np.int32))
        out = fuse.outputs(1, a.candidates, zeros=zeros)
        call = lambda: fuse.fuse_map_points_device(m, prm, T + 1, cap, n_pts, 1, 1, a.candidates, d_t, d_p, tgt, lst, cand, n_cand, out)
        shape = dict(items=1, candidates_per_item=int(n_cand.cpu()[0]), candidates_from_targets=from_targets)
    line = dict(tool="fuse_rate", step=step, n_kps=a.n_kps, **shape, **time_calls(s, call))
    if out is not None:
        st = out["status"].cpu().numpy()
        line["n_fused"] = int(out["n_fused"].sum())
        line["status_counts"] = np.bincount(st.reshape(-1), minlength=15).tolist()
    else:
        line["n_cand"] = int(n_again.cpu()[0])
    print(json.dumps(line), flush=True)
    m.close()


if __name__ == "__main__":
    main(__file__, STEPS, run_step, (("n-kps", 1000), ("targets", 40), ("list", 600), ("candidates", 25000)))

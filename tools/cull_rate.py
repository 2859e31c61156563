"""Time LocalMapping::KeyFrameCulling on the device -- msl_cull_keyframes on device-resident tables -- at the workload's shape: 200 keyframes
of 1000 keypoints along a trajectory (keyframe k holds points 125 k .. 125 k + 999, so a point has about 8 observations), one item of 30
candidates (the neighbours of a keyframe in the middle), and a batch of 64 items.  Beside it the wall time of the literal model's loop
(tests/cull_model.py: Python objects, only a sanity reference, not the reference's C++).  The rows of the two are compared before anything
is timed.
Clock: the device steps as tools/rate_common.py (HIP events on the handle's stream around the call, median of five after a warm-up); the
literal step time.perf_counter around cull_keyframes_literal, which builds its objects first, median of three.  Every step runs in a child
process of its own under a time limit, and the steps stop at the first that fails.  Prints one JSON line per step.
Kernel times: `rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/cull_rate.py --step device1` (a run of its
own; tracing slows the host, so the JSON line of that run is not the rate)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.rate_common import main, time_calls, to_device as dev, zeros  # noqa: E402
STEPS = ("device1", "device64", "literal1")
N_TAB, CAP, STEP, CCAP, TH_DEPTH = 200, 1000, 125, 30, 8.0


def workload(n_items, seed=1):
    """The arrays of msl.h for the trajectory map and n_items items spread along it, and the same map as the scene dict of
    tests/cull_model.py."""
    from manhattanslam_amd import KEYPOINT_DTYPE
    r = np.random.RandomState(seed)
    n_pts = STEP * (N_TAB - 1) + CAP
    held = (STEP * np.arange(N_TAB)[:, None] + np.arange(CAP)[None, :]).astype(np.int32)
    held[r.rand(N_TAB, CAP) < 0.1] = -1
    kps = np.zeros((N_TAB, CAP), KEYPOINT_DTYPE)
    kps["octave"] = r.choice([0, 1, 1, 2, 3], (N_TAB, CAP))
    uright = np.where(r.rand(N_TAB, CAP) < 0.7, 10.0, -1.0).astype(np.float32)
    depth = r.uniform(0.0, 9.0, (N_TAB, CAP)).astype(np.float32)
    k, i = np.nonzero(held >= 0)
    order = np.argsort(held[k, i], kind="stable")                          # by point, keyframes ascending inside a point
    k, i = k[order].astype(np.int32), i[order].astype(np.int32)
    p = held[k, i]
    off = np.zeros(n_pts + 1, np.int32)
    off[1:] = np.cumsum(np.bincount(p, minlength=n_pts))
    nobs = np.bincount(p, weights=np.where(uright[k, i] >= 0, 2, 1), minlength=n_pts).astype(np.int32)
    centre = np.linspace(40, 160, n_items).astype(int) if n_items > 1 else np.array([100])
    cand = np.stack([np.concatenate([c - 1 - np.arange(CCAP // 2), c + 1 + np.arange(CCAP // 2)]) for c in centre]).astype(np.int32)
    for row in cand:
        r.shuffle(row)
    a = dict(kps_un=kps, uright=uright, depth=depth, held_id=held, n_kps=np.full(N_TAB, CAP, np.int32),
             kf_flags=(1 | 2 * (r.rand(N_TAB) < 0.05)).astype(np.uint8), pt_flags=(r.rand(n_pts) > 0.05).astype(np.uint8), pt_nobs=nobs,
             obs_off=off, obs_kf=k, obs_idx=i, cand=cand, n_cand=np.full(n_items, CCAP, np.int32))
    scene = dict(held=[[None if x < 0 else int(x) for x in row] for row in held], octave=kps["octave"].tolist(), uright=uright.tolist(),
                 depth=depth.tolist(), kf_bad=[False] * N_TAB, not_erase=[bool(f & 2) for f in a["kf_flags"]],
                 pt_bad=[not f for f in a["pt_flags"]], pt_nobs=nobs.tolist(),
                 pt_obs=[list(zip(k[b:e].tolist(), i[b:e].tolist())) for b, e in zip(off[:-1], off[1:])], origin=0, th_depth=TH_DEPTH,
                 items=[[int(x) for x in row] for row in cand])
    return a, dict(n_pts=n_pts, n_obs_total=int(off[-1])), scene


def run_step(step, a_):
    import torch
    from manhattanslam_amd import cull, match
    from tests import cull_model as cm
    F = 64 if step.endswith("64") else 1
    a, sh, scene = workload(F)
    m = match.Matcher()
    s = torch.cuda.Stream()
    m.set_stream(s.cuda_stream)
    d = {k: dev(v) for k, v in a.items()}
    out = cull.keyframes_outputs(F, CCAP, zeros)
    params = cull.cull_params(TH_DEPTH)

    def device_call():
        cull.cull_keyframes_device(m, params, N_TAB, CAP, sh["n_pts"], F, sh["n_obs_total"], CCAP, 0, d, out)

    with torch.cuda.stream(s):
        device_call()
    m.sync()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    rows, order, _ = cm.cull_keyframes_literal(scene, scene["items"][0])   # the two agree before either is timed
    assert [tuple(int(got[k][0, j]) for k in ("n_mps", "n_redundant", "n_gone", "status")) for j in range(CCAP)] == rows
    shape = dict(items=F, keyframes=N_TAB, keypoints=CAP, candidates=CCAP, observations_per_point=round(sh["n_obs_total"] / sh["n_pts"], 2),
                 culled=float((got["status"] == cm.CULLED).sum(axis=1).mean()), mean_n_mps=float(got["n_mps"].mean()))
    if step.startswith("device"):
        t = time_calls(s, device_call)
    else:
        times = []
        for _ in range(3):
            t0 = time.perf_counter(); cm.cull_keyframes_literal(scene, scene["items"][0]); times.append((time.perf_counter() - t0) * 1e6)
        t = dict(us_per_call=round(float(np.median(times)), 2), us_calls=[round(x, 2) for x in times],
                 clock="time.perf_counter around cull_keyframes_literal, which builds its objects first; median of 3")
    print(json.dumps(dict(tool="cull_rate", step=step, **shape, us_per_item=round(t["us_per_call"] / F, 2), **t)), flush=True)
    m.close()


if __name__ == "__main__":
    main(__file__, STEPS, run_step, ())

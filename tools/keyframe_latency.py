"""Latency of msl_keyframe_decision and msl_points_3d in device memory on one matcher handle, by event pairs on the handle's stream (the
method of tools/plane_cloud_latency.py): one 640 x 480 frame of 1000 keypoints (40 keylines, 8 planes, a map of 20 000 points), and a batch
of 32 such frames.  msl_points_3d is measured in its three modes, the MSL_POINT3D_KEYFRAME call gated by the decision's need_kf as in the
chain.  One JSON line per measurement: the median, minimum and 90th percentile of `reps` calls in microseconds.  MSL_LIB selects a variant
library (tools/build_variant.sh) for an ablation."""
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from manhattanslam_amd import KEYPOINT_DTYPE, keyframe
from manhattanslam_amd.match import Matcher

N, NL, NP, N_PTS, N_LINES, N_TAB = 1000, 40, 8, 20000, 2000, 30
FX, FY, CX, CY, TH_DEPTH = 517.3, 516.5, 318.6, 255.3, 3.09


def frame(seed):
    """1000 keypoints over 640 x 480 with depths of 0.5 to 6 m (a tenth without depth), 60 % of the slots holding a map point."""
    rng = np.random.default_rng(seed)
    kps = np.zeros(N, KEYPOINT_DTYPE)
    kps["x"], kps["y"], kps["octave"], kps["class_id"] = rng.uniform(0, 640, N), rng.uniform(0, 480, N), rng.integers(0, 8, N), -1
    depth = rng.uniform(0.5, 6.0, N).astype(np.float32)
    depth[rng.random(N) < 0.1] = 0.0
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    Tcw = np.concatenate([q * np.sign(np.linalg.det(q)), rng.uniform(-1, 1, (3, 1))], 1).astype(np.float32)
    return dict(kps_un=kps, depth=depth, desc=rng.integers(0, 256, (N, 32), dtype=np.uint8), Tcw=Tcw,
                cur_held=np.where(rng.random(N) < 0.6, rng.integers(0, N_PTS, N), -1).astype(np.int32), outlier=(rng.random(N) < 0.1).astype(np.uint8),
                cur_lheld=np.where(rng.random(NL) < 0.6, rng.integers(0, N_LINES, NL), -1).astype(np.int32),
                line_outlier=(rng.random(NL) < 0.2).astype(np.uint8), plane_match=np.where(rng.random((NP, 3)) < 0.7, rng.integers(0, 20, (NP, 3)), -1).astype(np.int32),
                plane_outlier=(rng.random((NP, 3)) < 0.2).astype(np.uint8), flags=keyframe.TRACKED_LOCAL_MAP, frame_id=100 + seed, last_keyframe_id=60,
                last_reloc_frame_id=0, n_kfs=N_TAB, ref_kf=seed % N_TAB, local_mapping_idle=1)


def dev(a):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype.fields is not None:
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
    rng = np.random.default_rng(1)
    sf = 1.2 ** np.arange(8, dtype=np.float32)
    pprm, kprm = keyframe.point3d_params(FX, FY, CX, CY, TH_DEPTH, sf), keyframe.keyframe_params(30, 0, TH_DEPTH)
    s = torch.cuda.Stream()
    m = Matcher()
    m.set_stream(s.cuda_stream)
    z = lambda shape, dt: torch.zeros(shape, dtype=getattr(torch, np.dtype(dt).name), device="cuda")
    lib = os.environ.get("MSL_LIB", "product")
    table = dict(pt_nobs=rng.integers(0, 6, N_PTS).astype(np.int32), pt_flags=(rng.random(N_PTS) < 0.9).astype(np.uint8),
                 ln_nobs=rng.integers(0, 4, N_LINES).astype(np.int32), held_id=np.where(rng.random((N_TAB, N)) < 0.7, rng.integers(0, N_PTS, (N_TAB, N)), -1).astype(np.int32),
                 n_kps=np.full(N_TAB, N, np.int32))
    for F in (1, 32):
        frames = [frame(f) for f in range(F)]
        _, _, _, da = keyframe.pack_decision(frames, N, NL, NP)
        _, pa = keyframe.pack_points(frames, N)
        with torch.cuda.stream(s):
            d = {k: dev(v) for k, v in dict(da, **table).items()}
            do = keyframe.decision_outputs(F, N, NL, z)
            r = timed(s, lambda: keyframe.keyframe_decision_device(m, kprm, F, N, NL, NP, N_TAB, N_PTS, N_LINES, d, do), reps)
            print(json.dumps(dict(what="msl_keyframe_decision", frames=F, keypoints=N, need_kf=int(do["need_kf"].sum()), inliers=int(do["n_inliers"].sum()),
                                  lib=lib, **r)), flush=True)
            q = {k: dev(v) for k, v in pa.items()}
            q.update(pt_nobs=d["pt_nobs"], first_id=dev(np.arange(F, dtype=np.int32) * N + N_PTS))
            po = keyframe.points_outputs(F, N, z)
            for mode, name in ((keyframe.ALL, "ALL"), (keyframe.KEYFRAME, "KEYFRAME"), (keyframe.FRAME, "FRAME")):
                ins = dict(q, cur_held=do["held_out"], enable=do["need_kf"] if mode == keyframe.KEYFRAME else None)
                r = timed(s, lambda: keyframe.points_3d_device(m, pprm, F, N, N_PTS, mode, ins, po), reps)
                print(json.dumps(dict(what="msl_points_3d", mode=name, frames=F, keypoints=N, new=int(po["n_new"].sum()), walked=int(po["n_walked"].sum()),
                                      lib=lib, **r)), flush=True)
    m.sync()
    m.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 50)

"""Host mirror of Frame::GetLineDepth + Frame::Obtain3DLine (reference src/Frame.cc:179-186, :528-603, src/3DLineExtractor.cpp) and the line
half of their three call sites (src/Tracking.cc:575-592, :1107-1143, :1569-1618) through the C ABI: the world end points of the MapLines a
batch of frames creates (lines_3d), the device-memory form (lines_3d_device) and the per-keyline stage of the last call (debug_lines)."""
import numpy as np

from ._lib import LINE3D_PARAMS_DTYPE, MSL_MEM_DEVICE, MSL_MEM_HOST, call, check, lib, pad, ptr

ALL, INDEX_ORDER, DEPTH_ORDER = 0, 1, 2      # MSL_LINE3D_*: StereoInitialization, UpdateLastFrame, CreateNewKeyFrame
MAX_ITERATIONS = 64


def line3d_params(fx, fy, cx, cy, max_samples=100, min_points=10, max_iterations=10, max_new_lines=30, dist_thresh=1.5, min_support=0.4,
                  min_length=0.02):
    """msl_line3d_params: the camera and the constants of Obtain3DLine / extract3dline_mahdist / the call sites (defaults: the reference's)."""
    p = np.zeros(1, LINE3D_PARAMS_DTYPE)
    p["fx"], p["fy"], p["cx"], p["cy"] = fx, fy, cx, cy
    p["max_samples"], p["min_points"], p["max_iterations"], p["max_new_lines"] = max_samples, min_points, max_iterations, max_new_lines
    p["dist_thresh"], p["min_support"], p["min_length"] = dist_thresh, min_support, min_length
    return p


def pack_lines(frames, lcap=None):
    """Packs per-frame dicts into msl_lines_3d's arrays.  frame: line_ends (n, 4) f32, depth (H, W) f32, Tcw (3, 4) f32, seed (n,), and
    optionally line_flags (n,) u8.  Returns (lcap, width, height, dict of arrays named as in msl.h)."""
    lcap = lcap or max(max(len(f["line_ends"]) for f in frames), 1)
    H, W = frames[0]["depth"].shape
    depth = np.ascontiguousarray(np.stack([np.asarray(f["depth"], np.float32) for f in frames]))
    fr = [dict(f, line_flags=f.get("line_flags", np.zeros(len(f["line_ends"]), np.uint8)), seed=np.asarray(f["seed"], np.uint32)) for f in frames]
    return lcap, W, H, dict(line_ends=pad(fr, "line_ends", lcap, np.float32, shape=(4,)),
                            n_lines=np.array([len(f["line_ends"]) for f in frames], np.int32), depth=depth,
                            line_flags=pad(fr, "line_flags", lcap, np.uint8), Tcw=np.stack([np.asarray(f["Tcw"], np.float32).reshape(12) for f in frames]),
                            seed=pad(fr, "seed", lcap, np.uint32))


def lines_3d(params, frames, order=DEPTH_ORDER, device=0, handle=None, lcap=None):
    """msl_lines_3d on host arrays (synchronous); see pack_lines.  Returns a dict of the outputs, each [frames][lcap, ...]: line_depth
    (.., 2) f32, line_xyz (.., 6) f64, line_ok, line_new u8, n_support i32, and n_new [frames]."""
    lcap, W, H, a = pack_lines(frames, lcap)
    B = len(frames)
    out = dict(line_depth=np.zeros((B, lcap, 2), np.float32), line_xyz=np.zeros((B, lcap, 6), np.float64), line_ok=np.zeros((B, lcap), np.uint8),
               line_new=np.zeros((B, lcap), np.uint8), n_support=np.zeros((B, lcap), np.int32), n_new=np.zeros(B, np.int32))
    call("msl_lines_3d", handle, device, B, lcap, order, ptr(params), ptr(a["line_ends"]), ptr(a["n_lines"]), ptr(a["depth"]), 4 * W, 4 * W * H, W, H,
         ptr(a["line_flags"]), ptr(a["Tcw"]), ptr(a["seed"]), MSL_MEM_HOST, *[ptr(out[k]) for k in out], MSL_MEM_HOST)
    return out


def lines_3d_device(handle, params, n_frames, lcap, order, line_ends, n_lines, depth, depth_row_stride, depth_frame_stride, width, height,
                    line_flags, Tcw, seed, line_depth, line_xyz, line_ok, line_new, n_support, n_new):
    """Device-resident inputs and outputs (torch tensors / device pointers in msl.h's argument order; strides in bytes) on a match.Matcher:
    asynchronous on the handle's stream."""
    check(lib.msl_lines_3d(handle.h, n_frames, lcap, order, ptr(params), ptr(line_ends), ptr(n_lines), ptr(depth), depth_row_stride,
                           depth_frame_stride, width, height, ptr(line_flags), ptr(Tcw), ptr(seed), MSL_MEM_DEVICE, ptr(line_depth), ptr(line_xyz),
                           ptr(line_ok), ptr(line_new), ptr(n_support), ptr(n_new), MSL_MEM_DEVICE), "msl_lines_3d")


def debug_lines(handle, frame, line):
    """The per-keyline stage of the last lines_3d call on a match.Matcher: dict(n_kept, iters: [(i0, i1, count, record)], refits, ends (2,),
    m (3,), d (3,))."""
    counts = np.zeros(5, np.int32); its = np.zeros((MAX_ITERATIONS, 4), np.int32); md = np.zeros(6)
    check(lib.msl_lines_3d_debug(handle.h, frame, line, ptr(counts), ptr(its), ptr(md)), "msl_lines_3d_debug")
    return dict(n_kept=int(counts[0]), iters=[tuple(int(v) for v in r) for r in its[:counts[1]]], refits=int(counts[2]),
                ends=(int(counts[3]), int(counts[4])), m=md[:3].copy(), d=md[3:].copy())


__all__ = ["ALL", "INDEX_ORDER", "DEPTH_ORDER", "line3d_params", "pack_lines", "lines_3d", "lines_3d_device", "debug_lines"]

"""What the rate tools of the mapping entry points share (fuse_rate.py, linefuse_rate.py, mappoint_rate.py; triangulate_rate.py takes the
array helpers): numpy arrays to device tensors, device zeros by numpy dtype, the event clock and the runner that gives every step a child
process of its own."""
import argparse
import os
import subprocess
import sys

import numpy as np

CLOCK = "HIP events on the handle's stream around one call, median of 5 after a warm-up call"


def to_device(v):
    """A numpy array as a device tensor; a structured array as its bytes, one row per record."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(v.view(np.uint8).reshape(v.shape + (v.dtype.itemsize,)) if v.dtype.names else v)).cuda()


def zeros(shape, dt):
    """Device zeros of a numpy dtype (the `zeros` the outputs() builders of manhattanslam_amd take)."""
    import torch
    return torch.zeros(shape, dtype=getattr(torch, np.dtype(dt).name), device="cuda")


def time_calls(stream, call):
    """One warm-up call (the scratch grows there), then five calls each between two events on the stream.  Returns the fields of the JSON
    line: the median and the five times in microseconds, and the clock's description."""
    import torch
    times = []
    with torch.cuda.stream(stream):
        call()
        stream.synchronize()
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream); call(); e1.record(stream)
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3)
    return dict(us_per_call=round(float(np.median(times)), 2), us_calls=[round(x, 2) for x in times], clock=CLOCK)


def main(script, steps, run_step, options):
    """The command line every tool ends in.  options: the tool's own integer options as (name, default); --step runs one step here,
    --inline all of them here (for a profiler); otherwise every step gets a fresh child process under --step-timeout, and nothing more
    runs after a failure."""
    ap = argparse.ArgumentParser()
    for name, default in options:
        ap.add_argument("--" + name, type=int, default=default)
    ap.add_argument("--step", choices=steps)
    ap.add_argument("--inline", action="store_true", help="all steps in this process (for a profiler)")
    ap.add_argument("--step-timeout", type=float, default=120.0)
    a = ap.parse_args()
    if a.step:
        return run_step(a.step, a)
    if a.inline:
        for step in steps:
            run_step(step, a)
        return
    own = [x for name, _ in options for x in ("--" + name, str(getattr(a, name.replace("-", "_"))))]
    for step in steps:
        rc = subprocess.run([sys.executable, os.path.abspath(script), "--step", step] + own, timeout=a.step_timeout).returncode
        if rc != 0:
            sys.exit("step %s ended with %d" % (step, rc))

"""Host mirror of msl_observations_apply through the C ABI: a log of AddObservation / EraseObservation / SetBadFlag / Replace /
KeyFrame::SetBadFlag edits (reference src/MapPoint.cc:83-187, src/MapLine.cpp:75-172, src/KeyFrame.cc:185-197 and :362-368) executed in
order on the CSR observation table, the slots and the per-point arrays, and the new CSR table.  Every function takes the arrays under
msl.h's names (numpy arrays for host memory, torch tensors or anything with data_ptr() for device memory); with device memory on a
match.Matcher the call is asynchronous on the handle's stream."""
import numpy as np

from ._lib import MSL_MEM_DEVICE, MSL_MEM_HOST, RECORDS, call, ptr

OP_DTYPE = RECORDS["msl_obs_op"]
assert OP_DTYPE.itemsize == 16 and OP_DTYPE.names == ("op", "a", "b", "c")
ADD, ERASE, SET_BAD, REPLACE, KF_ERASE = 1, 2, 3, 4, 5                # MSL_OBS_*
CHANGED, TURNED_BAD = 1, 2                                            # op_status bits
OBS_MAX, MAX_OPS, MAX_KF_ERASE = 256, 65536, 256                      # MSL_OBS_MAX, MSL_OBS_MAX_OPS, MSL_OBS_MAX_KF_ERASE
MAX_TAB, MAX_CAP, MAX_PTS = 4096, 8192, 1 << 20
IN_KEYS = ("n_kps", "uright", "obs_off", "obs_kf", "obs_idx", "ops")
INOUT_KEYS = ("held_id", "pt_flags", "pt_nobs", "pt_ref", "pt_found", "pt_visible", "pt_replaced")
OUT_KEYS = ("obs_off_out", "obs_kf_out", "obs_idx_out", "op_status", "touched", "counts")


def pack_ops(ops):
    """The log as msl_obs_op records: `ops` is a sequence of (op, a, b, c), shorter tuples padded with 0 -- (ADD, id, keyframe, keypoint),
    (ERASE, id, keyframe), (SET_BAD, id), (REPLACE, id, survivor), (KF_ERASE, 0, keyframe)."""
    out = np.zeros(len(ops), OP_DTYPE)
    for o, rec in enumerate(ops):
        rec = tuple(rec) + (0,) * (4 - len(rec))
        out[o] = rec
    return out


def outputs(n_pts, n_ops, ocap, tcap, zeros=np.zeros):
    """The output arrays of one call, in msl.h's order (zeros(shape, dtype) allocates)."""
    return dict(obs_off_out=zeros((n_pts + 1,), np.int32), obs_kf_out=zeros((max(ocap, 1),), np.int32), obs_idx_out=zeros((max(ocap, 1),), np.int32),
                op_status=zeros((n_ops,), np.uint8), touched=zeros((tcap,), np.int32), counts=zeros((4,), np.int32))


def apply(n_tab, cap, n_pts, n_obs_total, n_ops, ocap, tcap, ins, inout, out, mem=MSL_MEM_HOST, device=0, handle=None):
    """msl_observations_apply: `ins` keyed by IN_KEYS (uright may be missing: every weight 1), `inout` by INOUT_KEYS (pt_found / pt_visible /
    pt_replaced may be missing), edited in place, `out` by OUT_KEYS; all in `mem` memory.  Returns out."""
    call("msl_observations_apply", handle, device, n_tab, cap, n_pts, n_obs_total, n_ops, ocap, tcap, *[ptr(ins.get(k)) for k in IN_KEYS],
         *[ptr(inout.get(k)) for k in INOUT_KEYS], mem, *[ptr(out.get(k)) for k in OUT_KEYS], mem)
    return out


def apply_device(handle, n_tab, cap, n_pts, n_obs_total, n_ops, ocap, tcap, ins, inout, out):
    """Device-resident tables on a match.Matcher: asynchronous on the handle's stream.  n_obs_total may be the capacity of obs_kf / obs_idx
    when the count of an earlier call has not been read back (msl.h)."""
    return apply(n_tab, cap, n_pts, n_obs_total, n_ops, ocap, tcap, ins, inout, out, MSL_MEM_DEVICE, handle=handle)


__all__ = ["pack_ops", "outputs", "apply", "apply_device", "OP_DTYPE", "IN_KEYS", "INOUT_KEYS", "OUT_KEYS"]

"""Host mirror of msl_connections_apply and msl_fuse_targets through the C ABI: a log of UpdateConnections / SetBadFlag edits (reference
src/KeyFrame.cc:113-145, :266-316, :349-448 and :455-467) executed in order on the weight maps, the ordered rows, the parents and the
keyframe flags, and vpTargetKFs of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:527-543).  Every function takes the arrays under
msl.h's names (numpy arrays for host memory, torch tensors or anything with data_ptr() for device memory); with device memory on a
match.Matcher the call is asynchronous on the handle's stream."""
import numpy as np

from ._lib import MSL_MEM_DEVICE, MSL_MEM_HOST, RECORDS, call, ptr

OP_DTYPE = RECORDS["msl_conn_op"]
assert OP_DTYPE.itemsize == 16 and OP_DTYPE.names == ("op", "a", "b", "c")
UPDATE, KF_BAD = 1, 2                                                 # MSL_CONN_*
DONE, PARENT_SET, EMPTY, ALREADY_BAD, KEPT = 1, 2, 4, 8, 16           # op_status
MAX_OPS, MAX_TAB = 4096, 4096                                         # MSL_CONN_MAX_OPS
LIVE, NOT_ERASE, CONNECTED = 1, 2, 4                                  # kf_flags bits
IN_KEYS = ("weight", "ops")
INOUT_KEYS = ("cw", "conn", "conn_w", "n_conn", "parent", "kf_flags")
OUT_KEYS = ("op_status", "touched", "counts")
TARGETS_IN_KEYS = ("conn", "n_conn", "kf_flags", "cur")
TARGETS_OUT_KEYS = ("targets", "n_targets")


def pack_ops(ops):
    """The log as msl_conn_op records: `ops` is a sequence of (op, a, b, c), shorter tuples padded with 0 -- (UPDATE, keyframe, weight row),
    (KF_BAD, keyframe)."""
    out = np.zeros(len(ops), OP_DTYPE)
    for o, rec in enumerate(ops):
        rec = tuple(rec) + (0,) * (4 - len(rec))
        out[o] = rec
    return out


def outputs(n_ops, tcap, zeros=np.zeros):
    """The output arrays of one msl_connections_apply call, in msl.h's order (zeros(shape, dtype) allocates)."""
    return dict(op_status=zeros((n_ops,), np.uint8), touched=zeros((tcap,), np.int32), counts=zeros((4,), np.int32))


def targets_outputs(n_items, tcap, zeros=np.zeros):
    """The output arrays of one msl_fuse_targets call."""
    return dict(targets=zeros((n_items, tcap), np.int32), n_targets=zeros((n_items,), np.int32))


def apply(n_tab, ccap, n_rows, n_ops, tcap, origin, th, ins, inout, out, mem=MSL_MEM_HOST, device=0, handle=None):
    """msl_connections_apply: `ins` keyed by IN_KEYS (weight missing or None when n_rows == 0), `inout` by INOUT_KEYS, edited in place,
    `out` by OUT_KEYS; all in `mem` memory.  Returns out."""
    call("msl_connections_apply", handle, device, n_tab, ccap, n_rows, n_ops, tcap, origin, th, *[ptr(ins.get(k)) for k in IN_KEYS],
         *[ptr(inout.get(k)) for k in INOUT_KEYS], mem, *[ptr(out.get(k)) for k in OUT_KEYS], mem)
    return out


def apply_device(handle, n_tab, ccap, n_rows, n_ops, tcap, origin, th, ins, inout, out):
    """Device-resident tables on a match.Matcher: asynchronous on the handle's stream."""
    return apply(n_tab, ccap, n_rows, n_ops, tcap, origin, th, ins, inout, out, MSL_MEM_DEVICE, handle=handle)


def fuse_targets(n_tab, ccap, n_items, nn, nn2, tcap, ins, out, mem=MSL_MEM_HOST, device=0, handle=None):
    """msl_fuse_targets: `ins` keyed by TARGETS_IN_KEYS, `out` by TARGETS_OUT_KEYS (the targets / n_targets msl_fuse_candidates takes); all
    in `mem` memory.  Returns out."""
    call("msl_fuse_targets", handle, device, n_tab, ccap, n_items, nn, nn2, tcap, *[ptr(ins.get(k)) for k in TARGETS_IN_KEYS], mem,
         *[ptr(out.get(k)) for k in TARGETS_OUT_KEYS], mem)
    return out


__all__ = ["pack_ops", "outputs", "targets_outputs", "apply", "apply_device", "fuse_targets", "OP_DTYPE", "IN_KEYS", "INOUT_KEYS", "OUT_KEYS",
           "TARGETS_IN_KEYS", "TARGETS_OUT_KEYS"]

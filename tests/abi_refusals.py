"""The refusal harness of the *_abi tests: call the device-indexed form of an entry on host arrays with one argument replaced, require
MSL_ERR_INVALID with every output (and in/out array) byte untouched, and hand back msl_last_error().  The argument order is read from
include/msl.h, so a test names arguments, never positions.  A plain module: no GPU, no fixture."""
import ctypes

import numpy as np

from tests.localmap_scenes import FILL, host_filled  # noqa: F401  (what the outputs hold before a call)

MSL_ERR_INVALID = -1


def _declarations():
    from manhattanslam_amd import _header
    return _header.declarations(_header.text("msl.h"))


def declared(entry):
    """The names of the int arguments and of the pointer arguments behind the first, as msl.h declares them."""
    decl = _declarations()[entry][1][1:]
    return [n for t, n in decl if t == "int"], [n for t, n in decl if t.endswith("*")]


def call(entry, ints, inputs, outputs, *, inout=(), **over):
    """(return code, msl_last_error()) of `entry`_batch.  ints: the int (and size_t) arguments by name; inputs: the arrays before `mem`, and
    the in/out arrays named in `inout`; outputs: the FILL-patterned arrays after `mem` (None: an optional one left out).  `over` replaces
    arguments: None is a NULL, an array goes in place, an int replaces an int, a callable edits a copy of the array.  An object handle
    (a ctypes.c_void_p) goes as it is.  device, mem and out_mem are 0 (device 0, host memory).  After a refusal the outputs must hold FILL
    and the in/out arrays their bytes."""
    from manhattanslam_amd import _lib
    ins = dict(inputs)
    for k in inout:                                                        # an accepted call writes them: the caller's scene stays as it is
        ins[k] = ins[k].copy()
    for k, v in over.items():
        if callable(v):
            ins[k] = ins[k].copy()
            v(ins[k])
    before = {k: ins[k].tobytes() for k in inout}
    args, behind_mem = [], False
    for _, n in _declarations()[entry + "_batch"][1]:
        behind_mem = behind_mem or n == "mem"
        if n in over and not callable(over[n]):
            v = over[n]
        elif n in ("device", "mem", "out_mem"):
            v = 0
        elif n in ints:
            v = ints[n]
        else:
            v = outputs[n] if behind_mem and n in outputs else ins[n]
        args.append(v if isinstance(v, (int, ctypes.c_void_p)) else _lib.ptr(v))
    rc = getattr(_lib.lib, entry + "_batch")(*args)
    if rc == MSL_ERR_INVALID:
        assert all((v.view(np.uint8) == FILL).all() for v in outputs.values() if v is not None), (entry, over)
        assert all(ins[k].tobytes() == v for k, v in before.items()), (entry, over)
    return rc, _lib.lib.msl_last_error().decode()


def refused(entry, ints, inputs, outputs, *, inout=(), **over):
    """msl_last_error() of a call (see `call`) that must be refused: on a machine without a device too, since the check comes first."""
    rc, msg = call(entry, ints, inputs, outputs, inout=inout, **over)
    assert rc == MSL_ERR_INVALID, (entry, over, rc, msg)
    return msg


def put(index, value):
    """The edit x[index] = value (index: a position or a field name)."""
    def edit(x):
        x[index] = value
    return edit


def both(field, hi, top=None):
    """A limit 1 .. hi (top: how the message writes hi) from both sides."""
    top = top or str(hi)
    return [(field, 0, f"{field} 0 outside 1 .. {top}"), (field, hi + 1, f"{field} {hi + 1} outside 1 .. {top}")]

"""ctypes binding of include/msl.h and include/msl_debug.h, read from the two headers at import (_header.py).  Fails loudly when libmsl.so has
not been built."""
import ctypes as C
import os

import numpy as np

from . import _header
from ._header import MslError  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MSL_LIB", os.path.join(_HERE, "libmsl.so"))   # MSL_LIB: kernel-variant experiments only

_API, _DEBUG = _header.text("msl.h"), _header.text("msl_debug.h")

# struct name -> numpy dtype with the header's layout (nested members flattened in place)
RECORDS = _header.records(_API)
KEYPOINT_DTYPE = RECORDS["msl_keypoint"]
SURFEL_DTYPE = RECORDS["msl_surfel"]
SEED_DTYPE = RECORDS["msl_seed"]
PEAC_STATS_DTYPE = RECORDS["msl_peac_stats"]
PEAC_PARAMS_DTYPE = RECORDS["msl_peac_params"]
PEAC_BLOCK_DTYPE = RECORDS["msl_peac_block"]
PEAC_PLANE_DTYPE = RECORDS["msl_peac_plane"]
FRAME_PARAMS_DTYPE = RECORDS["msl_frame_params"]
MATCH_PARAMS_DTYPE = RECORDS["msl_match_params"]
LOCAL_MATCH_PARAMS_DTYPE = RECORDS["msl_local_match_params"]
LOCAL_TRACK_DTYPE = RECORDS["msl_local_track"]
LINE_MATCH_PARAMS_DTYPE = RECORDS["msl_line_match_params"]
KEYLINE_DTYPE = RECORDS["msl_keyline"]
LINE_TRACK_DTYPE = RECORDS["msl_line_track"]
POSE_PARAMS_DTYPE = RECORDS["msl_pose_params"]
PLANE_PARAMS_DTYPE = RECORDS["msl_plane_params"]
PLANE_CLOUD_PARAMS_DTYPE = RECORDS["msl_plane_cloud_params"]
BOW_MATCH_PARAMS_DTYPE = RECORDS["msl_bow_match_params"]
KEYFRAME_MATCH_PARAMS_DTYPE = RECORDS["msl_keyframe_match_params"]
PNP_PARAMS_DTYPE = RECORDS["msl_pnp_params"]
LINE3D_PARAMS_DTYPE = RECORDS["msl_line3d_params"]
TRIANGULATE_PARAMS_DTYPE = RECORDS["msl_triangulate_params"]
FUSE_PARAMS_DTYPE = RECORDS["msl_fuse_params"]
REFRESH_PARAMS_DTYPE = RECORDS["msl_refresh_params"]
LINE_FUSE_PARAMS_DTYPE = RECORDS["msl_line_fuse_params"]
assert LINE_FUSE_PARAMS_DTYPE.itemsize == 112
assert LINE3D_PARAMS_DTYPE.itemsize == 56 and TRIANGULATE_PARAMS_DTYPE.itemsize == 176 and FUSE_PARAMS_DTYPE.itemsize == 180 and REFRESH_PARAMS_DTYPE.itemsize == 68
assert PNP_PARAMS_DTYPE.itemsize == 120 and PNP_PARAMS_DTYPE.fields["probability"][1] == 88
assert POSE_PARAMS_DTYPE.itemsize == 152 and KEYPOINT_DTYPE.itemsize == 28 and SURFEL_DTYPE.itemsize == 56 and SEED_DTYPE.itemsize == 64

MSL_MEM_HOST, MSL_MEM_DEVICE = 0, 1

# name -> (restype, argtypes); every symbol include/msl.h and include/msl_debug.h declare
SIGNATURES = {name: _header.ctypes_of(decl, name) for src in (_API, _DEBUG) for name, decl in _header.declarations(src).items()}
_DEFINES = _header.defines(_DEBUG)
MSL_ORB_NKERNELS = _DEFINES["MSL_ORB_NKERNELS"]
MSL_SF_NKERNELS = _DEFINES["MSL_SF_NKERNELS"]


def _load():
    # PyTorch-ROCm bundles its own libamdhip64; when torch shares the process it must be loaded first so that both
    # sides bind one HIP runtime (two runtimes in one process cannot both own the GPU).  C/C++ hosts are unaffected.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise MslError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(make -C manhattanslam_amd/csrc). There is no CPU fallback.")
    dll = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(dll, name)  # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    return dll


lib = _load()


def check(rc, what="msl call"):
    if rc != 0:
        raise MslError(f"{what} failed ({rc}): {lib.msl_last_error().decode()}")


def device_count():
    return int(lib.msl_device_count())


def ptr(a):
    """void* of a numpy array (host) or anything exposing data_ptr() (torch device tensor)."""
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr())
    return a.ctypes.data_as(C.c_void_p)


def pad(frames, key, cap, dtype, fill=0, shape=()):
    """frames[f][key] (per frame: at most cap rows of `shape`) as the ABI's [frames][cap, *shape] layout, padded with fill."""
    out = np.full((len(frames), cap) + shape, fill, dtype)
    for f, fr in enumerate(frames):
        out[f, :len(fr[key])] = fr[key]
    return out


def fill_levels(p, **tables):
    """nlevels and the per-level tables (field name = values, all of one length) of a params record; tables longer than the record's 16
    entries are left unfilled for the library to refuse."""
    n = len(next(iter(tables.values())))
    p["nlevels"] = n
    if n <= 16:
        for k, v in tables.items():
            p[k][0, :n] = v


def call(name, handle, device, *args):
    """The handle form `name` on handle.h when a handle is given, else `name`_batch on the device's shared one."""
    if handle is not None:
        check(getattr(lib, name)(handle.h, *args), name)
    else:
        check(getattr(lib, name + "_batch")(device, *args), name + "_batch")

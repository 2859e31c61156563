"""Host mirror of a keyframe that is born with planes, through the C ABI: keyframe_planes is the plane loop of CreateNewKeyFrame (reference
src/Tracking.cc:1620-1645) and of StereoInitialization (:594-602) with the plane members of the KeyFrame constructor and SetPose
(src/KeyFrame.cc:50-52, 74-86); manhattan_observe is the plane part of LocalMapping::ProcessNewKeyFrame (src/LocalMapping.cc:160-218) with
Map::Add[Partial]ManhattanObservation (src/Map.cc:247-275).  Every function takes the arrays under msl.h's names (numpy arrays for host
memory, torch tensors or anything with data_ptr() for device memory) and writes the in/out arrays and outputs it is given; with device memory
on a match.Matcher the call is asynchronous on the handle's stream."""
import numpy as np

from . import plane
from ._lib import MSL_MEM_DEVICE, MSL_MEM_HOST, RECORDS, call, pad, ptr
from .plane import MAX_FCAP, MAX_FRAMES, MAX_KCAP, MAX_MCAP, MAX_PCAP, MAX_QCAP   # the chain's limits stand in plane

KFPLANES_FRAME_DTYPE = RECORDS["msl_kfplanes_frame"]
assert KFPLANES_FRAME_DTYPE.itemsize == 16

KEYFRAME, INIT = 0, 1                                                 # MSL_KFPLANES_*: mode
SKIPPED, HELD, NEW, NO_ROOM = 0, 1, 2, 3                              # MSL_KFPLANES_*: status
FULL_NO_ROOM, PART_NO_ROOM = 1, 2                                     # MSL_MANHATTAN_*_NO_ROOM: msl_manhattan_observe's status
PLANES_IN_KEYS = ("frames", "plane_coef", "plane_npts", "n_planes", "Tcw", "plane_outlier")
PLANES_INOUT_KEYS = ("plane_match", "mp_w", "mp_flags", "mp_first_kf", "n_map", "kf_Rwc", "kf_coef", "kf_npts")
PLANES_OUT_KEYS = ("kf_plane_match", "plane_new", "obs_add", "merge_into", "Twc", "n_new", "set_not_erase", "status")
OBSERVE_IN_KEYS = ("frames", "kf_plane_match", "plane_coef", "n_planes", "mp_flags", "mp_first_kf", "n_map")
OBSERVE_INOUT_KEYS = ("full_tab", "n_full", "part_tab", "n_part")
OBSERVE_OUT_KEYS = ("added_full", "added_part", "set_not_erase", "recent_plane", "status")


def frame_records(frames):
    """msl_kfplanes_frame records from dicts with enable (default 1), kf_slot, kf_id."""
    r = np.zeros(len(frames), KFPLANES_FRAME_DTYPE)
    for f, fr in enumerate(frames):
        r["enable"][f], r["kf_slot"][f], r["kf_id"][f] = fr.get("enable", 1), fr["kf_slot"], fr["kf_id"]
    return r


def pack(frames, pcap=None, mcap=None, fcap=None, qcap=None, kcap=None):
    """Packs per-frame dicts into the arrays of both entries.  frame: enable, kf_slot, kf_id, plane_coef (K,4) f32, plane_npts (K,) i32,
    Tcw (12,) f32, plane_match (K,3) i32, plane_outlier (K,3) u8, mp_w (M,4) f32, mp_flags (M,) u8, mp_first_kf (M,) i32, and as in
    plane.pack_manhattan full (E,7) / part (E,5) i32 (any order: sorted here), kf_Rwc (R,9) f32, kf_coef: R arrays (Q,4), kf_npts: R arrays
    (Q,).  Returns (caps (pcap, mcap, fcap, qcap, kcap), dict of arrays named as in msl.h)."""
    (pcap, mcap, fcap, qcap, kcap), m = plane.pack_manhattan(frames, pcap, mcap, fcap, qcap, kcap)
    coef, npts, n_planes, match, flags, n_map, ft, nf, pt, nq, kR, kc, kn = m
    a = dict(frames=frame_records(frames), plane_coef=coef, plane_npts=npts, n_planes=n_planes,
             Tcw=np.stack([np.asarray(f["Tcw"], np.float32).reshape(12) for f in frames]),
             plane_outlier=pad(frames, "plane_outlier", pcap, np.uint8, shape=(3,)), plane_match=match,
             mp_w=pad(frames, "mp_w", mcap, np.float32, shape=(4,)), mp_flags=flags, mp_first_kf=pad(frames, "mp_first_kf", mcap, np.int32),
             n_map=n_map, kf_Rwc=kR, kf_coef=kc, kf_npts=kn, full_tab=ft, n_full=nf, part_tab=pt, n_part=nq)
    return (pcap, mcap, fcap, qcap, kcap), a


def planes_outputs(n_frames, pcap, zeros=np.zeros):
    """The output arrays of one msl_keyframe_planes call, in msl.h's order (zeros(shape, dtype) allocates)."""
    F = n_frames
    return dict(kf_plane_match=zeros((F, pcap, 3), np.int32), plane_new=zeros((F, pcap), np.uint8), obs_add=zeros((F, pcap, 3), np.uint8),
                merge_into=zeros((F, pcap), np.int32), Twc=zeros((F, 12), np.float64), n_new=zeros((F,), np.int32),
                set_not_erase=zeros((F,), np.int32), status=zeros((F, pcap), np.int32))


def observe_outputs(n_frames, pcap, zeros=np.zeros):
    """The output arrays of one msl_manhattan_observe call, in msl.h's order."""
    F = n_frames
    return dict(added_full=zeros((F,), np.int32), added_part=zeros((F,), np.int32), set_not_erase=zeros((F,), np.int32),
                recent_plane=zeros((F, pcap), np.uint8), status=zeros((F,), np.int32))


def keyframe_planes(n_frames, pcap, mcap, kcap, mode, arrays, out=None, mem=MSL_MEM_HOST, device=0, handle=None):
    """msl_keyframe_planes: `arrays` keyed by PLANES_IN_KEYS and PLANES_INOUT_KEYS (the map-plane table, the keyframe rows and, in INIT mode,
    plane_match are edited in place), `out` by PLANES_OUT_KEYS (allocated on the host when None); all in `mem` memory.  Returns out."""
    out = planes_outputs(n_frames, pcap) if out is None else out
    call("msl_keyframe_planes", handle, device, n_frames, pcap, mcap, kcap, mode, *[ptr(arrays.get(k)) for k in PLANES_IN_KEYS], mem,
         *[ptr(arrays.get(k)) for k in PLANES_INOUT_KEYS], *[ptr(out.get(k)) for k in PLANES_OUT_KEYS], mem)
    return out


def keyframe_planes_device(handle, n_frames, pcap, mcap, kcap, mode, arrays, out):
    """Device-resident arrays on a match.Matcher: asynchronous on the handle's stream."""
    return keyframe_planes(n_frames, pcap, mcap, kcap, mode, arrays, out, MSL_MEM_DEVICE, handle=handle)


def manhattan_observe(params, n_frames, pcap, mcap, fcap, qcap, kcap, arrays, out=None, mem=MSL_MEM_HOST, device=0, handle=None):
    """msl_manhattan_observe: params = plane.plane_params(...) (mf_ver_th is read); `arrays` keyed by OBSERVE_IN_KEYS and OBSERVE_INOUT_KEYS
    (the two tables and their counts are edited in place), `out` by OBSERVE_OUT_KEYS; all in `mem` memory.  Returns out."""
    out = observe_outputs(n_frames, pcap) if out is None else out
    call("msl_manhattan_observe", handle, device, n_frames, pcap, mcap, fcap, qcap, kcap, ptr(params), *[ptr(arrays.get(k)) for k in OBSERVE_IN_KEYS],
         mem, *[ptr(arrays.get(k)) for k in OBSERVE_INOUT_KEYS], *[ptr(out.get(k)) for k in OBSERVE_OUT_KEYS], mem)
    return out


def manhattan_observe_device(handle, params, n_frames, pcap, mcap, fcap, qcap, kcap, arrays, out):
    """Device-resident arrays on a match.Matcher: asynchronous on the handle's stream."""
    return manhattan_observe(params, n_frames, pcap, mcap, fcap, qcap, kcap, arrays, out, MSL_MEM_DEVICE, handle=handle)


__all__ = ["KEYFRAME", "INIT", "SKIPPED", "HELD", "NEW", "NO_ROOM", "FULL_NO_ROOM", "PART_NO_ROOM", "PLANES_IN_KEYS", "PLANES_INOUT_KEYS",
           "PLANES_OUT_KEYS", "OBSERVE_IN_KEYS", "OBSERVE_INOUT_KEYS", "OBSERVE_OUT_KEYS", "frame_records", "pack", "planes_outputs",
           "observe_outputs", "keyframe_planes", "keyframe_planes_device", "manhattan_observe", "manhattan_observe_device"]

"""Scenes for msl_keyframe_planes and msl_manhattan_observe (tests/kfplanes_model.py is the model).  Test infrastructure only.

A frame is a dict of manhattanslam_amd.kfplanes.pack: enable, kf_slot, kf_id, plane_coef (K,4), plane_npts (K,), Tcw (12,), plane_match
(K,3), plane_outlier (K,3), the map-plane table mp_w / mp_flags / mp_first_kf, the Manhattan tables full / part and the keyframe rows
kf_Rwc / kf_coef / kf_npts, with mp_clouds (empty) so that plane.pack_associate takes it too."""
import numpy as np

from tests import kfplanes_model as kp

F32 = np.float32
TH = 0.1                                                                     # Plane.MFVerticalThreshold of the scenes
FILL = 0x5A
PCAP, MCAP, FCAP, QCAP, KCAP = 13, 40, 160, 120, 5                            # the ragged batch's capacities


def pose(rng):
    """rows 0-2 of a rigid Tcw, (12,) f32."""
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    q *= np.sign(np.linalg.det(q))
    return np.concatenate([q, rng.uniform(-2, 2, (3, 1))], 1).astype(F32).reshape(12)


def axis_coef(rng, axis, noise=0.02):
    """A plane whose normal is near +-axis: planes of different axes pass the gate at TH, planes of one axis do not."""
    n = rng.normal(0, noise, 3)
    n[axis] = rng.choice([-1.0, 1.0])
    n /= np.linalg.norm(n)
    return np.append(n, rng.uniform(-3, 3)).astype(F32)


def frame(rng, K, n_map, axes=None, slot=0, kf_id=7, enable=1, n_kf=KCAP):
    """K frame planes over a map of n_map rows; nothing held yet.  The keyframe rows hold FILL-like junk so that a written row shows."""
    axes = [k % 3 for k in range(K)] if axes is None else axes
    return dict(enable=enable, kf_slot=slot, kf_id=kf_id, plane_coef=np.array([axis_coef(rng, x) for x in axes], F32).reshape(K, 4),
                plane_npts=rng.integers(4, 500, K).astype(np.int32), Tcw=pose(rng), plane_match=np.full((K, 3), -1, np.int32),
                plane_outlier=np.zeros((K, 3), np.uint8), mp_w=rng.normal(size=(n_map, 4)).astype(F32), mp_flags=np.ones(n_map, np.uint8),
                mp_first_kf=rng.integers(0, 6, n_map).astype(np.int32), mp_clouds=[np.zeros((0, 3), F32)] * n_map,
                full=np.zeros((0, 7), np.int32), part=np.zeros((0, 5), np.int32), kf_Rwc=rng.normal(size=(n_kf, 9)).astype(F32),
                kf_coef=[rng.normal(size=(PCAP, 4)).astype(F32) for _ in range(n_kf)],
                kf_npts=[rng.integers(1, 99, PCAP).astype(np.int32) for _ in range(n_kf)])


def foreign(rng, rows, n, w, kf=1):
    """n distinct table entries over the map rows `rows` (none need be held by a frame plane), unsorted."""
    keys = set()
    while len(keys) < n:
        keys.add(tuple(sorted(rng.choice(rows, w, replace=False).tolist())))
    return np.array([list(k) + [kf] + rng.integers(0, PCAP, w).tolist() for k in sorted(keys, key=lambda k: rng.random())], np.int32).reshape(-1, 2 * w + 1)


def unique(tab, w):
    """The entries of a table whose key no earlier entry has."""
    seen, out = set(), []
    for e in np.asarray(tab, np.int32).tolist():
        if tuple(e[:w]) not in seen:
            seen.add(tuple(e[:w]))
            out.append(e)
    return np.array(out, np.int32).reshape(-1, 2 * w + 1)


def ragged():
    """Nine frames with 0, 1, 2, 3, 5, 12, 5, 5, 12 planes: the cases of the issue, one or more per frame."""
    rng = np.random.default_rng(9100)
    fr = []
    f = frame(rng, 0, 3, slot=1)                                              # 0: no planes, tables pre-filled: nothing changes but the keyframe row
    f["full"], f["part"] = foreign(rng, np.arange(3), 1, 3), foreign(rng, np.arange(3), 3, 2)
    fr.append(f)
    fr.append(frame(rng, 1, 4, slot=0))                                       # 1: one plane, not held, no outlier: new; empty tables stay empty
    f = frame(rng, 2, 6, slot=4)                                              # 2: a held plane and a held plane whose outlier byte is set:
    f["plane_match"][:, 0] = [2, 5]                                           #    both observed (:1628 does not ask), one pair
    f["plane_outlier"][1, 0] = 1
    f["plane_match"][1, 1:] = [3, 4]                                          #    its parallel / vertical observations are not made
    fr.append(f)
    f = frame(rng, 3, 9, slot=2)                                              # 3: three held planes, the first possible triple; every new key
    f["plane_match"][:, 0] = [8, 0, 4]                                        #    sorts after every old entry
    f["full"], f["part"] = np.array([[0, 1, 2, 1, 3, 4, 5]], np.int32), np.array([[0, 1, 1, 6, 7], [0, 3, 0, 1, 2]], np.int32)
    fr.append(f)
    f = frame(rng, 5, 10, axes=[0, 1, 2, 1, 0], slot=3, kf_id=5)              # 4: held, not held + outlier, new, two planes on one row in slot 0,
    f["plane_match"][:, 0] = [6, -1, -1, 2, 6]                                #    rows repeated in the parallel and the vertical slots
    f["plane_outlier"][1, 0] = 1
    f["plane_match"][:, 1] = [1, 7, 1, 1, -1]
    f["plane_match"][:, 2] = [-1, 3, 3, -1, 3]
    f["mp_first_kf"][[6, 2]] = [5, 4]                                         #    row 6 is recent for this keyframe, row 2 is not
    f["part"] = np.array([[6, 2, 0, 9, 9]], np.int32)                         #    a key the keyframe names is in the table already: kept
    fr.append(f)
    f = frame(rng, 12, 30, slot=0, kf_id=3)                                   # 5: twelve held planes on the odd rows, a bad one among them,
    f["plane_match"][:, 0] = 1 + 2 * np.arange(12)                            #    foreign entries before, between and after the new keys, and
    f["mp_flags"][7] = 0                                                      #    two keys of the keyframe present already
    f["full"] = np.concatenate([foreign(rng, np.arange(0, 30, 2), 14, 3), foreign(rng, np.arange(24, 30), 6, 3),
                                [[1, 3, 5, 2, 0, 0, 0], [3, 5, 13, 2, 1, 1, 1], [0, 1, 2, 1, 0, 0, 0], [21, 23, 29, 1, 0, 0, 0]]]).astype(np.int32)
    f["full"] = unique(f["full"], 3)
    f["part"] = np.concatenate([foreign(rng, np.arange(0, 30, 2), 12, 2), [[1, 3, 2, 5, 5], [0, 1, 1, 0, 0], [23, 29, 1, 0, 0]]]).astype(np.int32)
    f["part"] = unique(f["part"], 2)
    fr.append(f)
    f = frame(rng, 5, 10, slot=2, enable=0)                                   # 6: not enabled: every in/out array keeps its bytes
    f["plane_match"][:, 0] = [1, -1, 2, -1, 3]
    f["full"], f["part"] = foreign(rng, np.arange(10), 5, 3), foreign(rng, np.arange(10), 5, 2)
    fr.append(f)
    f = frame(rng, 5, MCAP - 1, slot=1)                                       # 7: mcap exhausted in mid-frame: one new row, then NO_ROOM twice
    f["plane_match"][:, 0] = [4, -1, 9, -1, -1]                               #    the new triple and the first new pair sort before every old entry:
    f["full"] = np.array([[5, 6, 7, 0, 1, 2, 3], [10, 11, 12, 2, 0, 0, 0]], np.int32)   # every old entry moves and the whole table is copied back
    f["part"] = np.array([[4, 10, 0, 8, 9], [30, 31, 2, 0, 1]], np.int32)
    fr.append(f)
    f = frame(rng, 12, 30, slot=4)                                            # 8: both tables with exactly one free row: NO_ROOM, bytes untouched
    f["plane_match"][:, 0] = 2 * np.arange(12)
    f["full"], f["part"] = foreign(rng, np.arange(1, 30, 2), FCAP - 1, 3), foreign(rng, np.arange(30), QCAP - 1, 2)
    fr.append(f)
    return fr


def expected(arrays, mode, th=TH, fill=None):
    """The model chained on copies of packed arrays: msl_keyframe_planes, then msl_manhattan_observe on what it left.  Returns (arrays after,
    planes outputs, observe outputs).  fill: a function (shape, dtype) for the outputs' bytes before the call."""
    a = {k: v.copy() for k, v in arrays.items()}
    F, pcap = a["plane_coef"].shape[:2]
    po, oo = kp.planes_outputs(F, pcap), kp.observe_outputs(F, pcap)
    if fill is not None:
        po, oo = {k: fill(v.shape, v.dtype) for k, v in po.items()}, {k: fill(v.shape, v.dtype) for k, v in oo.items()}
    kp.keyframe_planes(mode, a, po)
    kp.manhattan_observe(th, dict(a, kf_plane_match=po["kf_plane_match"]), a["kf_Rwc"].shape[1], oo)
    return a, po, oo


def host_filled(shape, dtype):
    return np.frombuffer(bytes([FILL]) * (int(np.prod(shape)) * np.dtype(dtype).itemsize), dtype).reshape(shape).copy()


# ---- random plane graphs carried over many keyframes (tests/test_kfplanes_model.py) ---------------------------------------------------------
def random_keyframe(rng, n_rows, K):
    """The references of one random frame over a map of n_rows rows: (coef (K,4), npts, Tcw, match (K,3), outlier (K,))."""
    coef = np.array([axis_coef(rng, int(rng.integers(0, 3)), noise=0.05) for _ in range(K)], F32).reshape(K, 4)
    match = np.full((K, 3), -1, np.int32)
    for k in range(K):
        for s in range(3):
            if n_rows and rng.random() < (0.6, 0.3, 0.3)[s]:
                match[k, s] = rng.integers(0, min(n_rows, 6)) if rng.random() < 0.4 else rng.integers(0, n_rows)   # rows held twice are common
    return coef, rng.integers(4, 500, K).astype(np.int32), pose(rng), match, (rng.random(K) < 0.25).astype(np.uint8)

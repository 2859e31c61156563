"""Sequential CPU models of a keyframe that is born with planes, the parity reference of msl_keyframe_planes and msl_manhattan_observe.
Test infrastructure only.

The literal twin works on an object graph as the reference does: MapPlane with its three observation maps (src/MapPlane.cc:48-68), KeyFrame
with its three plane vectors and its pose (src/KeyFrame.cc:50-52, 74-86), Map with the map planes in creation order and the two Manhattan
maps keyed by frozensets (src/Map.cc:32-123 hashes and compares the keys as unordered sets).  create_keyframe is the plane loop of
Tracking::CreateNewKeyFrame (src/Tracking.cc:1620-1645) or, in INIT mode, of StereoInitialization (:594-602); process_new_keyframe is
LocalMapping::ProcessNewKeyFrame (src/LocalMapping.cc:160-218).

The array form (keyframe_planes, manhattan_observe) restates the same on the ABI's arrays, in place, and is what the kernels are compared
with; tests/test_kfplanes_model.py asserts it equal to the twin.  manhattan_observe keeps its keys in dictionaries, so it is usable at 64
planes and 65536-entry tables.

Types as the reference has them: ComputePlaneWorldCoeff is plane_match_model.world_coef; Ow = -Rwc * tcw is mappoint_model.camera_centre (one
cv::gemm: double accumulation, alpha = -1, one rounding); the Twc of msl_map_plane_merge is the float Twc widened; the angles are float dot
products, left to right, gated by angle < th && angle > -th."""
import numpy as np

from tests import mappoint_model as mm
from tests import plane_match_model as pm

F32 = np.float32
KEYFRAME, INIT = 0, 1
SKIPPED, HELD, NEW, NO_ROOM = 0, 1, 2, 3
FULL_NO_ROOM, PART_NO_ROOM = 1, 2


def pose_inverse(Tcw):
    """(Rwc (3,3) f32, Twc (12,) f64): KeyFrame::SetPose, and Converter::toMatrix4d(GetPoseInverse()) rows 0-2."""
    T = np.asarray(Tcw, F32).reshape(3, 4)
    Rwc = np.ascontiguousarray(T[:, :3].T)
    return Rwc, np.concatenate([Rwc, mm.camera_centre(T).reshape(3, 1)], 1).astype(np.float64).reshape(12)


def vertical(a, b, th):
    """The gate of src/LocalMapping.cc:192 / :209 on two coefficient rows."""
    angle = a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    return bool(angle < th and angle > -th)


# ---- the literal twin ----------------------------------------------------------------------------------------------------------------------
class MapPlane:
    def __init__(self, mnId, world, first_kf):
        self.mnId, self.world, self.mnFirstKFid, self.bad = mnId, np.asarray(world, F32), first_kf, False
        self.obs, self.par_obs, self.ver_obs = {}, {}, {}

    def AddObservation(self, kf, idx, which="obs"):
        m = getattr(self, which)
        if kf in m:                                                       # src/MapPlane.cc:50, :58, :65
            return False
        m[kf] = idx
        return True

    def GetIndexInKeyFrame(self, kf):
        return self.obs.get(kf, -1)


class KeyFrame:
    def __init__(self, mnId, slot, frame):
        """The plane members of KeyFrame(Frame&, ...): copies of the frame's, and SetPose."""
        self.mnId, self.slot = mnId, slot
        self.coef, self.npts = np.array(frame["plane_coef"], F32).reshape(-1, 4), np.array(frame["plane_npts"], np.int32)
        self.planes, self.par, self.ver = list(frame["planes"]), list(frame["par"]), list(frame["ver"])
        self.Rwc, self.Twc = pose_inverse(frame["Tcw"])
        self.not_erase = False


class Map:
    def __init__(self):
        self.planes, self.full, self.part = [], {}, {}                    # GetAllMapPlanes() order = creation order (pinned)

    def AddManhattanObservation(self, p1, p2, p3, kf):
        key = frozenset((p1.mnId, p2.mnId, p3.mnId))
        if key in self.full:
            return
        kf.not_erase = True
        self.full[key] = (kf, (p1, p2, p3))

    def AddPartialManhattanObservation(self, p1, p2, kf):
        key = frozenset((p1.mnId, p2.mnId))
        if key in self.part:
            return
        kf.not_erase = True
        self.part[key] = (kf, (p1, p2))

    def tables(self):
        """The two maps flattened as plane.sort_full / sort_part take them: {a, b, c, kf, ia, ib, ic}, {a, b, kf, ia, ib}."""
        full = [[p.mnId for p in ps] + [kf.slot] + [p.GetIndexInKeyFrame(kf) for p in ps] for kf, ps in self.full.values()]
        part = [[p.mnId for p in ps] + [kf.slot] + [p.GetIndexInKeyFrame(kf) for p in ps] for kf, ps in self.part.values()]
        return np.array(full, np.int32).reshape(-1, 7), np.array(part, np.int32).reshape(-1, 5)


def create_keyframe(world, frame, mnId, slot, mode, mcap=1 << 30):
    """frame: plane_coef, plane_npts, Tcw, planes / par / ver (lists of MapPlane or None), outlier (K,) mvbPlaneOutlier.  Returns
    (KeyFrame, dict plane_new, obs_add (K,3), status, set_not_erase).  In INIT mode the frame's planes[i] becomes the new plane (:601).
    mcap: the rows the map-plane table has (the ABI's limit, not the reference's)."""
    kf = KeyFrame(mnId, slot, frame)
    K = len(kf.coef)
    rec = dict(plane_new=np.zeros(K, np.uint8), obs_add=np.zeros((K, 3), np.uint8), status=np.zeros(K, np.int32), set_not_erase=0)
    for i in range(K):
        if mode == KEYFRAME:
            if frame["par"][i] is not None and not frame["outlier"][i]:                                  # :1621-1623
                rec["obs_add"][i, 1] = frame["par"][i].AddObservation(kf, i, "par_obs")
            if frame["ver"][i] is not None and not frame["outlier"][i]:                                  # :1624-1626
                rec["obs_add"][i, 2] = frame["ver"][i].AddObservation(kf, i, "ver_obs")
            if frame["planes"][i] is not None:                                                           # :1628-1631
                rec["obs_add"][i, 0] = frame["planes"][i].AddObservation(kf, i)
                rec["status"][i] = HELD
                continue
            if frame["outlier"][i]:                                                                      # :1633-1635
                continue
            rec["set_not_erase"] = 1                                                                     # :1637
        if len(world.planes) >= mcap:
            rec["status"][i] = NO_ROOM
            continue
        p3D = pm.world_coef(frame["Tcw"], kf.coef[i])                                                    # :1639 / :595
        pNewMP = MapPlane(len(world.planes), p3D, mnId)
        rec["obs_add"][i, 0] = pNewMP.AddObservation(kf, i)
        kf.planes[i] = pNewMP                                                                            # AddMapPlane
        world.planes.append(pNewMP)
        rec["plane_new"][i], rec["status"][i] = 1, NEW
        if mode == INIT:
            frame["planes"][i] = pNewMP                                                                  # :601
    return kf, rec


def process_new_keyframe(world, kf, th):
    """src/LocalMapping.cc:160-218.  Returns recent (K,) u8: the mlpRecentAddedMapPlanes pushes."""
    th = F32(th)
    K = len(kf.coef)
    recent = np.zeros(K, np.uint8)
    for i, pMP in enumerate(kf.planes):                                                                  # :162-170
        if pMP is None or pMP.bad:
            continue
        if pMP.mnFirstKFid == kf.mnId:
            recent[i] = 1
    for i in range(K):
        pMP1 = kf.planes[i]
        if pMP1 is None or pMP1.bad:
            continue
        for j in range(i + 1, K):
            pMP2 = kf.planes[j]
            if pMP2 is None or pMP2.bad or pMP2.mnId == pMP1.mnId:
                continue
            if vertical(kf.coef[i], kf.coef[j], th):
                for k in range(j + 1, K):
                    pMP3 = kf.planes[k]
                    if pMP3 is None or pMP3.bad or pMP3.mnId == pMP1.mnId or pMP3.mnId == pMP2.mnId:
                        continue
                    if vertical(kf.coef[i], kf.coef[k], th) and vertical(kf.coef[j], kf.coef[k], th):
                        world.AddManhattanObservation(pMP1, pMP2, pMP3, kf)
                world.AddPartialManhattanObservation(pMP1, pMP2, kf)
    return recent


# ---- the array form --------------------------------------------------------------------------------------------------------------------------
def planes_outputs(F, pcap):
    return dict(kf_plane_match=np.zeros((F, pcap, 3), np.int32), plane_new=np.zeros((F, pcap), np.uint8), obs_add=np.zeros((F, pcap, 3), np.uint8),
                merge_into=np.zeros((F, pcap), np.int32), Twc=np.zeros((F, 12), np.float64), n_new=np.zeros(F, np.int32),
                set_not_erase=np.zeros(F, np.int32), status=np.zeros((F, pcap), np.int32))


def keyframe_planes(mode, a, out=None):
    """msl_keyframe_planes on the ABI's arrays (dict `a` under msl.h's names; the in/out arrays are edited in place, so pass copies).  `out`
    holds the outputs' bytes before the call (rows at and beyond n_planes keep them); zeros when None.  Returns out."""
    F, pcap = a["plane_coef"].shape[:2]
    mcap, kcap = a["mp_w"].shape[1], a["kf_Rwc"].shape[1]
    out = planes_outputs(F, pcap) if out is None else out
    for f in range(F):
        enable, slot, kf_id = (int(a["frames"][n][f]) for n in ("enable", "kf_slot", "kf_id"))
        on = enable != 0 and 0 <= slot < kcap
        n = min(max(int(a["n_planes"][f]), 0), pcap)
        nmap = min(max(int(a["n_map"][f]), 0), mcap)
        match = np.where((a["plane_match"][f, :n] >= 0) & (a["plane_match"][f, :n] < nmap), a["plane_match"][f, :n], -1)
        out["kf_plane_match"][f, :n] = match
        out["plane_new"][f, :n], out["obs_add"][f, :n], out["merge_into"][f, :n], out["status"][f, :n] = 0, 0, -1, SKIPPED
        out["Twc"][f] = pose_inverse(a["Tcw"][f])[1]
        out["n_new"][f] = out["set_not_erase"][f] = 0
        if not on:
            continue
        rows, seen = nmap, [set(), set(), set()]
        for k in range(n):
            o0 = a["plane_outlier"][f, k, 0] != 0
            if mode == KEYFRAME:
                for s in (1, 2):
                    if match[k, s] >= 0 and not o0 and match[k, s] not in seen[s]:
                        seen[s].add(int(match[k, s]))
                        out["obs_add"][f, k, s] = 1
                if match[k, 0] >= 0:
                    out["status"][f, k] = HELD
                    if match[k, 0] not in seen[0]:
                        seen[0].add(int(match[k, 0]))
                        out["obs_add"][f, k, 0] = 1
                    continue
                if o0:
                    continue
                out["set_not_erase"][f] = 1
            if rows >= mcap:
                out["status"][f, k] = NO_ROOM
                continue
            a["mp_w"][f, rows] = pm.world_coef(a["Tcw"][f], a["plane_coef"][f, k])
            a["mp_flags"][f, rows], a["mp_first_kf"][f, rows] = 1, kf_id
            out["kf_plane_match"][f, k, 0] = out["merge_into"][f, k] = rows
            out["plane_new"][f, k], out["obs_add"][f, k, 0], out["status"][f, k] = 1, 1, NEW
            if mode == INIT:
                a["plane_match"][f, k, 0] = rows
            rows += 1
        out["n_new"][f] = rows - nmap
        if rows > nmap:
            a["n_map"][f] = rows
        a["kf_Rwc"][f, slot] = pose_inverse(a["Tcw"][f])[0].reshape(9)
        a["kf_coef"][f, slot], a["kf_npts"][f, slot] = 0, 0
        a["kf_coef"][f, slot, :n], a["kf_npts"][f, slot, :n] = a["plane_coef"][f, :n], a["plane_npts"][f, :n]
    return out


def observe_outputs(F, pcap):
    return dict(added_full=np.zeros(F, np.int32), added_part=np.zeros(F, np.int32), set_not_erase=np.zeros(F, np.int32),
                recent_plane=np.zeros((F, pcap), np.uint8), status=np.zeros(F, np.int32))


def _merge(tab, n_old, cap, new):
    """The table with the entries of `new` (key tuple -> entry) merged in by key, or None when it has no room for them all."""
    w = len(tab[0]) // 2
    if n_old + len(new) > cap:
        return None
    rows = sorted([tuple(int(x) for x in e) for e in tab[:n_old]] + list(new.values()), key=lambda e: e[:w])
    return np.array(rows, np.int32).reshape(-1, 2 * w + 1)


def manhattan_observe(th, a, kcap, out=None):
    """msl_manhattan_observe on the ABI's arrays (full_tab / n_full / part_tab / n_part edited in place).  Returns out."""
    F, pcap = a["plane_coef"].shape[:2]
    mcap, fcap, qcap = a["mp_flags"].shape[1], a["full_tab"].shape[1], a["part_tab"].shape[1]
    out = observe_outputs(F, pcap) if out is None else out
    th = F32(th)
    for f in range(F):
        enable, slot, kf_id = (int(a["frames"][n][f]) for n in ("enable", "kf_slot", "kf_id"))
        on = enable != 0 and 0 <= slot < kcap
        n = min(max(int(a["n_planes"][f]), 0), pcap)
        nmap = min(max(int(a["n_map"][f]), 0), mcap)
        held = []
        for k in range(n):
            m = int(a["kf_plane_match"][f, k, 0])
            held.append(m if on and 0 <= m < nmap and (a["mp_flags"][f, m] & 1) else -1)
            out["recent_plane"][f, k] = 1 if held[k] >= 0 and a["mp_first_kf"][f, held[k]] == kf_id else 0
        first = {}
        for k in range(n):
            if held[k] >= 0:
                first.setdefault(held[k], k)
        c = a["plane_coef"][f, :n, :3].astype(F32)
        with np.errstate(invalid="ignore", over="ignore"):
            G = (c[:, None, 0] * c[None, :, 0] + c[:, None, 1] * c[None, :, 1]) + c[:, None, 2] * c[None, :, 2]
            ok = (G < th) & (G > -th)
        nf, nq = min(max(int(a["n_full"][f]), 0), fcap), min(max(int(a["n_part"][f]), 0), qcap)
        old_full = {tuple(e[:3]) for e in a["full_tab"][f, :nf].tolist()}
        old_part = {tuple(e[:2]) for e in a["part_tab"][f, :nq].tolist()}
        new_full, new_part = {}, {}
        for i in range(n):
            if held[i] < 0:
                continue
            for j in range(i + 1, n):
                if held[j] < 0 or held[j] == held[i] or not ok[i, j]:
                    continue
                for k in range(j + 1, n):
                    if held[k] < 0 or held[k] == held[i] or held[k] == held[j] or not ok[i, k] or not ok[j, k]:
                        continue
                    key = tuple(sorted((held[i], held[j], held[k])))
                    if key not in old_full and key not in new_full:
                        new_full[key] = key + (slot,) + tuple(first[r] for r in key)
                key = tuple(sorted((held[i], held[j])))
                if key not in old_part and key not in new_part:
                    new_part[key] = key + (slot,) + tuple(first[r] for r in key)
        status = 0
        full, part = _merge(a["full_tab"][f], nf, fcap, new_full), _merge(a["part_tab"][f], nq, qcap, new_part)
        if full is None:
            status, new_full = status | FULL_NO_ROOM, {}
        elif new_full:
            a["full_tab"][f, :len(full)], a["n_full"][f] = full, len(full)
        if part is None:
            status, new_part = status | PART_NO_ROOM, {}
        elif new_part:
            a["part_tab"][f, :len(part)], a["n_part"][f] = part, len(part)
        out["added_full"][f], out["added_part"][f], out["status"][f] = len(new_full), len(new_part), status
        out["set_not_erase"][f] = 1 if new_full or new_part else 0
    return out

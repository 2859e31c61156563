"""The sequential model of msl_connections_apply and msl_fuse_targets, and their literal twins on Python objects.

The array model works on the arrays of include/msl.h: a state is a dict of cw[n][n], conn[n][ccap], conn_w[n][ccap], n_conn[n], parent[n]
(int32) and kf_flags[n] (uint8); `apply` executes a log on a copy and returns the state it leaves with op_status, touched and counts.
The twin restates src/KeyFrame.cc statement by statement on objects -- dict maps iterated in pointer order (= table index), ordered
vectors, children sets, mpParent, mbFirstConnection -- with the two pins of msl.h (a second SetBadFlag and an UpdateConnections on a bad
keyframe do nothing; a NULL mpParent is not dereferenced).  An object graph has no ccap: the twin equals the arrays with ccap == n_tab."""
import numpy as np

UPDATE, KF_BAD = 1, 2
DONE, PARENT_SET, EMPTY, ALREADY_BAD, KEPT = 1, 2, 4, 8, 16
MAX_OPS, MAX_TAB = 4096, 4096
LIVE, NOT_ERASE, CONNECTED = 1, 2, 4
STATE_KEYS = ("cw", "conn", "conn_w", "n_conn", "parent", "kf_flags")


def pad(op):
    return tuple(op) + (0,) * (4 - len(op))


def empty(n_tab, ccap=None, flags=None):
    """n_tab new keyframes without a connection: flags == 1 (or `flags`)."""
    ccap = n_tab if ccap is None else ccap
    return dict(cw=np.zeros((n_tab, n_tab), np.int32), conn=np.full((n_tab, ccap), -1, np.int32), conn_w=np.zeros((n_tab, ccap), np.int32),
                n_conn=np.zeros(n_tab, np.int32), parent=np.full(n_tab, -1, np.int32),
                kf_flags=np.full(n_tab, LIVE, np.uint8) if flags is None else np.array(flags, np.uint8))


def copy(state):
    return {k: np.array(state[k]) for k in STATE_KEYS}


def same_state(a, b):
    return all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in STATE_KEYS)


# ---- the array model -----------------------------------------------------------------------------------------------------------------------
def ordered(w, idx):
    """(weights, indices) by descending weight, equal weights by descending index: sort of pair<int, KeyFrame*> and push_front."""
    w, idx = np.asarray(w, np.int64), np.asarray(idx, np.int64)
    order = np.lexsort((idx, w))[::-1]
    return w[order], idx[order]


def rebuilt(row):
    """UpdateBestCovisibles: every entry of a cw row that is present."""
    row = np.asarray(row)
    idx = np.nonzero(row > 0)[0]
    return ordered(row[idx], idx)


def store(s, j, pairs):
    """The ordered row of j: what fits ccap, the full count."""
    w, idx = pairs
    m = min(len(idx), s["conn"].shape[1])
    s["conn"][j], s["conn_w"][j] = -1, 0
    s["conn"][j][:m], s["conn_w"][j][:m] = idx[:m], w[:m]
    s["n_conn"][j] = len(idx)


def _update(s, k, W, origin, th, touched, events):
    n = len(s["parent"])
    if not s["kf_flags"][k] & LIVE:
        return ALREADY_BAD
    W = np.maximum(np.asarray(W, np.int64), 0)
    W[k] = 0
    if not W.any():
        return EMPTY
    sel = np.nonzero(W >= th)[0]
    if not len(sel):
        sel = np.array([np.argmax(W)])                                         # nmax, pKFmax by strict > in ascending order: the first maximum
    for j in sel:                                                         # AddConnection
        j = int(j)
        if s["cw"][j][k] != W[j]:
            s["cw"][j][k] = W[j]
            pairs = rebuilt(s["cw"][j])
            if len(pairs[0]) > 1 and (pairs[0] < th).any():
                events.add("below th in a rebuilt row")
            store(s, j, pairs)
            touched.add(j)
        else:
            events.add("equal weight")
    s["cw"][k] = W
    store(s, k, ordered(W[sel], sel))
    touched.add(k)
    st = DONE
    if not s["kf_flags"][k] & CONNECTED and k != origin:
        s["parent"][k] = s["conn"][k][0]
        s["kf_flags"][k] |= CONNECTED
        st |= PARENT_SET
    return st


def _bad(s, a, origin, touched, events, tally):
    n, ccap = s["conn"].shape
    if a == origin or s["kf_flags"][a] & NOT_ERASE:
        return KEPT
    if not s["kf_flags"][a] & LIVE:
        return ALREADY_BAD
    keeps = (s["cw"][:, a] > 0) & (s["cw"][a] <= 0) & (s["kf_flags"] & LIVE != 0)
    keeps[a] = False
    if keeps.any():                                                       # a live keyframe holds a, a never held it: nothing erases that entry
        events.add("stale bad neighbour")
    for j in np.nonzero((s["cw"][a] > 0) & (s["cw"][:, a] > 0))[0]:         # EraseConnection
        j = int(j)
        if j != a:
            s["cw"][j][a] = 0
            store(s, j, rebuilt(s["cw"][j]))
            touched.add(j)
    s["cw"][a] = 0
    store(s, a, ordered([], []))
    pa = int(s["parent"][a])
    cands = {pa} if 0 <= pa < n else set()
    children = [int(c) for c in np.nonzero((s["parent"] == a) & (s["kf_flags"] & LIVE != 0))[0] if c != a]
    while children:
        best, pick = -1, None
        for c in children:
            for pos in range(min(max(int(s["n_conn"][c]), 0), ccap)):
                e = int(s["conn"][c][pos])
                if 0 <= e < n and e in cands:
                    w = max(int(s["cw"][c][e]), 0)
                    if w > best:
                        best, pick = w, (c, e)
        if pick is None:
            break
        c, e = pick
        if e != pa:
            events.add("chained re-parenting")
        s["parent"][c] = e
        cands.add(c); children.remove(c); touched.add(c)
        tally[1] += 1
    for c in children:
        events.add("leftover child")
        s["parent"][c] = pa
        touched.add(c)
        tally[1] += 1
    s["kf_flags"][a] &= ~LIVE & 0xFF
    touched.add(a)
    tally[0] += 1
    return DONE


def apply(state, weight, ops, origin=-1, th=15, tcap=None, events=None):
    """The log on a copy of `state`: dict(state, op_status, touched, counts).  weight: the rows an UPDATE names (a sequence of rows of
    n_tab weights).  An op with an unknown code or a field outside its table has status 0 and does nothing (the device-memory contract)."""
    s = copy(state)
    n, ccap = s["conn"].shape
    touched, tally, status = set(), [0, 0], []
    events = set() if events is None else events
    for op in ops:
        code, a, b, _ = pad(op)
        st = 0
        if code == UPDATE and 0 <= a < n and 0 <= b < len(weight):
            st = _update(s, a, weight[b], origin, th, touched, events)
        elif code == KF_BAD and 0 <= a < n:
            st = _bad(s, a, origin, touched, events, tally)
        status.append(st)
    touched = sorted(touched)
    over = sum(1 for j in touched if s["n_conn"][j] > ccap)
    return dict(state=s, op_status=status, touched=touched, counts=[len(touched), tally[0], tally[1], over])


def fuse_targets(conn, n_conn, kf_flags, cur, nn=10, nn2=5):
    """vpTargetKFs per current keyframe, in push order (the full list: the ABI drops what is beyond tcap)."""
    n, ccap = conn.shape
    best = lambda k, m: [int(x) for x in conn[k][:min(max(int(n_conn[k]), 0), ccap, m)]]
    live = lambda k: 0 <= k < n and bool(kf_flags[k] & LIVE)
    out = []
    for c in cur:
        targets, stamped = [], set()
        for k1 in (best(c, nn) if 0 <= c < n else []):
            if not live(k1) or k1 in stamped:
                continue
            targets.append(k1); stamped.add(k1)
            targets += [k2 for k2 in best(k1, nn2) if live(k2) and k2 not in stamped and k2 != c]
        out.append(targets)
    return out


# ---- the literal twin ----------------------------------------------------------------------------------------------------------------------
class KeyFrame:
    """The graph half of the reference's KeyFrame.  mnId is the table index, and pointer order is mnId order."""

    def __init__(self, idx, is_origin=False, not_erase=False):
        self.mnId, self.is_origin = idx, is_origin
        self.mConnectedKeyFrameWeights = {}
        self.mvpOrderedConnectedKeyFrames, self.mvOrderedWeights = [], []
        self.mbFirstConnection, self.mpParent, self.mspChildrens = True, None, set()
        self.mbNotErase, self.mbBad = not_erase, False
        self.mnFuseTargetForKF = None

    def _map(self):
        """map<KeyFrame*, int> in iteration order"""
        return sorted(self.mConnectedKeyFrameWeights.items(), key=lambda it: it[0].mnId)

    def AddConnection(self, pKF, weight):
        if pKF not in self.mConnectedKeyFrameWeights:
            self.mConnectedKeyFrameWeights[pKF] = weight
        elif self.mConnectedKeyFrameWeights[pKF] != weight:
            self.mConnectedKeyFrameWeights[pKF] = weight
        else:
            return
        self.UpdateBestCovisibles()

    def UpdateBestCovisibles(self):
        vPairs = [(w, kf.mnId, kf) for kf, w in self._map()]
        vPairs.sort(key=lambda p: (p[0], p[1]))
        lKFs, lWs = [], []
        for w, _, kf in vPairs:
            lKFs.insert(0, kf); lWs.insert(0, w)
        self.mvpOrderedConnectedKeyFrames, self.mvOrderedWeights = lKFs, lWs

    def UpdateConnections(self, KFcounter, th=15):
        """From :266 on; KFcounter is the map the counting loops built ({KeyFrame: count}, no zero entries, never this keyframe)."""
        if self.mbBad:                                                    # pin
            return
        if not KFcounter:
            return
        nmax, pKFmax, vPairs = 0, None, []
        for kf, w in sorted(KFcounter.items(), key=lambda it: it[0].mnId):
            if w > nmax:
                nmax, pKFmax = w, kf
            if w >= th:
                vPairs.append((w, kf.mnId, kf))
                kf.AddConnection(self, w)
        if not vPairs:
            vPairs.append((nmax, pKFmax.mnId, pKFmax))
            pKFmax.AddConnection(self, nmax)
        vPairs.sort(key=lambda p: (p[0], p[1]))
        lKFs, lWs = [], []
        for w, _, kf in vPairs:
            lKFs.insert(0, kf); lWs.insert(0, w)
        self.mConnectedKeyFrameWeights = dict(KFcounter)
        self.mvpOrderedConnectedKeyFrames, self.mvOrderedWeights = lKFs, lWs
        if self.mbFirstConnection and not self.is_origin:
            self.mpParent = self.mvpOrderedConnectedKeyFrames[0]
            self.mpParent.mspChildrens.add(self)
            self.mbFirstConnection = False

    def ChangeParent(self, pKF):
        self.mpParent = pKF
        if pKF is not None:                                               # pin: the reference dereferences NULL
            pKF.mspChildrens.add(self)

    def GetWeight(self, pKF):
        return self.mConnectedKeyFrameWeights.get(pKF, 0)

    def EraseConnection(self, pKF):
        if pKF in self.mConnectedKeyFrameWeights:
            del self.mConnectedKeyFrameWeights[pKF]
            self.UpdateBestCovisibles()

    def SetBadFlag(self):
        """The connection and tree half; returns whether it ran."""
        if self.is_origin or self.mbNotErase:
            return False
        if self.mbBad:                                                    # pin
            return False
        for kf, _ in self._map():
            kf.EraseConnection(self)
        self.mConnectedKeyFrameWeights = {}
        self.mvpOrderedConnectedKeyFrames, self.mvOrderedWeights = [], []
        sParentCandidates = set() if self.mpParent is None else {self.mpParent}
        while self.mspChildrens:
            bContinue, mx, pC, pP = False, -1, None, None
            for pKF in sorted(self.mspChildrens, key=lambda k: k.mnId):
                if pKF.mbBad:
                    continue
                for con in pKF.mvpOrderedConnectedKeyFrames:
                    for cand in sorted(sParentCandidates, key=lambda k: k.mnId):
                        if con.mnId == cand.mnId:
                            w = pKF.GetWeight(con)
                            if w > mx:
                                pC, pP, mx, bContinue = pKF, con, w, True
            if bContinue:
                pC.ChangeParent(pP)
                sParentCandidates.add(pC)
                self.mspChildrens.discard(pC)
            else:
                break
        for kf in sorted(self.mspChildrens, key=lambda k: k.mnId):
            kf.ChangeParent(self.mpParent)
        if self.mpParent is not None:
            self.mpParent.mspChildrens.discard(self)
        self.mbBad = True
        return True


def twin_objects(n_tab, origin=-1, flags=None):
    return [KeyFrame(k, k == origin, bool(flags is not None and flags[k] & NOT_ERASE)) for k in range(n_tab)]


def twin_from_state(s, origin=-1):
    """The objects of a consistent array state with ccap == n_tab."""
    n = len(s["parent"])
    assert s["conn"].shape[1] == n
    kfs = twin_objects(n, origin, s["kf_flags"])
    for k, kf in enumerate(kfs):
        kf.mbBad, kf.mbFirstConnection = not s["kf_flags"][k] & LIVE, not s["kf_flags"][k] & CONNECTED
        kf.mConnectedKeyFrameWeights = {kfs[j]: int(w) for j, w in enumerate(s["cw"][k]) if w > 0}
        m = int(s["n_conn"][k])
        kf.mvpOrderedConnectedKeyFrames, kf.mvOrderedWeights = [kfs[int(j)] for j in s["conn"][k][:m]], s["conn_w"][k][:m].tolist()
        if s["parent"][k] >= 0:
            kf.mpParent = kfs[int(s["parent"][k])]
            if not kf.mbBad:
                kf.mpParent.mspChildrens.add(kf)
    return kfs


def twin_step(kfs, op, weight, th=15):
    """One op on the objects, as the caller of the reference would make it."""
    code, a, b, _ = pad(op)
    if code == UPDATE:
        counter = {kfs[j]: int(w) for j, w in enumerate(weight[b]) if j != a and w > 0}
        kfs[a].UpdateConnections(counter, th)
    elif code == KF_BAD:
        kfs[a].SetBadFlag()


def twin_differences(kfs, s):
    """What differs between the objects and an array state with ccap == n_tab (an empty list: nothing)."""
    n = len(kfs)
    diff = []
    for k, kf in enumerate(kfs):
        if {o.mnId: w for o, w in kf.mConnectedKeyFrameWeights.items()} != {j: int(w) for j, w in enumerate(s["cw"][k]) if w != 0}:
            diff.append(("cw", k))
        m = int(s["n_conn"][k])
        if [o.mnId for o in kf.mvpOrderedConnectedKeyFrames] != s["conn"][k][:m].tolist() or kf.mvOrderedWeights != s["conn_w"][k][:m].tolist():
            diff.append(("conn", k))
        if (s["conn"][k][m:] != -1).any() or (s["conn_w"][k][m:] != 0).any():
            diff.append(("beyond the count", k))
        if (-1 if kf.mpParent is None else kf.mpParent.mnId) != s["parent"][k]:
            diff.append(("parent", k))
        if kf.mbBad != (not s["kf_flags"][k] & LIVE) or kf.mbFirstConnection != (not s["kf_flags"][k] & CONNECTED):
            diff.append(("flags", k))
        if not kf.mbBad and {c.mnId for c in kf.mspChildrens} != {c for c in range(n) if s["parent"][c] == k and s["kf_flags"][c] & LIVE}:
            diff.append(("children", k))
    return diff


def fuse_targets_literal(conn, n_conn, kf_flags, cur, nn=10, nn2=5):
    """LocalMapping::SearchInNeighbors :527-543 on objects, one fresh set of stamps per current keyframe."""
    n, ccap = conn.shape
    out = []
    for item, c in enumerate(cur):
        kfs = twin_objects(n)
        for k, kf in enumerate(kfs):
            kf.mbBad = not kf_flags[k] & LIVE
            kf.mvpOrderedConnectedKeyFrames = [kfs[int(x)] for x in conn[k][:min(int(n_conn[k]), ccap)]]
        best = lambda kf, m: kf.mvpOrderedConnectedKeyFrames[:m]          # GetBestCovisibilityKeyFrames
        cur_kf, vpTargetKFs = kfs[c], []
        for pKFi in best(cur_kf, nn):
            if pKFi.mbBad or pKFi.mnFuseTargetForKF == cur_kf.mnId:
                continue
            vpTargetKFs.append(pKFi)
            pKFi.mnFuseTargetForKF = cur_kf.mnId
            for pKFi2 in best(pKFi, nn2):
                if pKFi2.mbBad or pKFi2.mnFuseTargetForKF == cur_kf.mnId or pKFi2.mnId == cur_kf.mnId:
                    continue
                vpTargetKFs.append(pKFi2)
        out.append([kf.mnId for kf in vpTargetKFs])
    return out

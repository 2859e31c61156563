"""Scenes for the local-map entries: random keyframe graphs and hand-built ones (tests/localmap_model.py describes the scene dict), their
packing into the ABI's arrays with mappoint.pack_table / pack_observations, the arrays the model expects of a call, and the three calls."""
import numpy as np

from tests import localmap_model as lm

FILL = 0x5A                                                           # what the outputs hold before a call


def graph(n_tab, conn=None, parent=None, kf_bad=()):
    """A scene of n_tab keyframes without map elements: conn / parent as dicts over the keyframes that have any."""
    return dict(kf_bad=[k in kf_bad for k in range(n_tab)], conn=[list((conn or {}).get(k, [])) for k in range(n_tab)],
                parent=[(parent or {}).get(k) for k in range(n_tab)], held=[[] for _ in range(n_tab)], lheld=[[] for _ in range(n_tab)],
                pt_bad=[], pt_nobs=[], pt_obs=[], ln_bad=[False], ln_nobs=[1], frames=[])


def add_point(scene, observers, bad=False, nobs=None):
    """A point observed by `observers`, each holding it in a new slot; returns its id."""
    p = len(scene["pt_bad"])
    scene["pt_bad"].append(bad); scene["pt_obs"].append(list(observers)); scene["pt_nobs"].append(len(observers) if nobs is None else nobs)
    for k in observers:
        scene["held"][k].append(p)
    return p


def vote_scene(n_tab, votes, **kw):
    """graph(...) with one frame whose slots give keyframe k votes[k] votes: one point per voted keyframe, held votes[k] times."""
    s = graph(n_tab, **kw)
    held = []
    for k, v in sorted(votes.items()):
        held += [add_point(s, [k])] * v
    s["frames"].append(dict(held=held, lheld=[], prev=[]))
    return s


def stop_scene(first):
    """130 keyframes of which the first `first` get a vote; each has three neighbours outside the list, all but keyframe 0 a parent outside
    it, keyframes 0 and 1 children outside it."""
    parent = {k: 129 - (k % 2) for k in range(1, first)}
    parent.update({103: 0, 104: 1, 105: 1})
    return vote_scene(130, {k: 1 for k in range(first)}, conn={k: [100 + (k % 3), 110 + k % 7, 120] for k in range(first)}, parent=parent)


def random_scene(seed, n_tab, cap, n_pts, frame_sizes, klcap=3, lcap=3, n_lines=7, ccap=None, bad=0.12):
    rng = np.random.default_rng(seed)
    ccap = ccap or n_tab
    s = graph(n_tab)
    s["kf_bad"] = [bool(rng.random() < bad) for _ in range(n_tab)]
    s["parent"] = [None if k == 0 or rng.random() < 0.25 else int(rng.integers(0, k)) for k in range(n_tab)]
    for k in range(n_tab):
        others = [j for j in rng.permutation(n_tab) if j != k]
        s["conn"][k] = [int(j) for j in others[:min(int(rng.choice([0, 3, 12, 25])), ccap, len(others))]]
    s["pt_bad"] = [bool(rng.random() < bad) for _ in range(n_pts)]
    s["pt_obs"] = [[] for _ in range(n_pts)]
    s["held"] = [[None] * int(rng.integers(0, cap + 1)) for _ in range(n_tab)]
    for p in range(n_pts):
        for k in rng.permutation(n_tab)[:int(rng.integers(0, 5))]:
            free = [i for i, q in enumerate(s["held"][k]) if q is None]
            if free:
                s["held"][k][int(rng.choice(free))] = p
                s["pt_obs"][p].append(int(k))
    for k in range(n_tab):                                            # slots that repeat a point of the keyframe, or hold one without an observation
        for i, q in enumerate(s["held"][k]):
            if q is None and rng.random() < 0.2:
                s["held"][k][i] = int(rng.integers(0, n_pts))
    s["pt_nobs"] = [0 if rng.random() < 0.15 else len(o) for o in s["pt_obs"]]
    s["ln_bad"] = [bool(rng.random() < bad) for _ in range(n_lines)]
    s["ln_nobs"] = [int(rng.integers(0, 3)) for _ in range(n_lines)]
    s["lheld"] = [[None if rng.random() < 0.3 else int(rng.integers(0, n_lines)) for _ in range(int(rng.integers(0, klcap + 1)))] for _ in range(n_tab)]
    for n in frame_sizes:
        s["frames"].append(dict(held=[None if rng.random() < 0.2 else int(rng.integers(0, n_pts)) for _ in range(n)],
                                lheld=[None if rng.random() < 0.3 else int(rng.integers(0, n_lines)) for _ in range(int(rng.integers(0, lcap + 1)))],
                                prev=[int(k) for k in rng.permutation(n_tab)[:int(rng.integers(0, min(n_tab, 6) + 1))]]))
    return s


def _rows(lists, cap):
    out = np.full((len(lists), cap), -1, np.int32)
    for r, l in enumerate(lists):
        out[r, :len(l)] = [-1 if x is None else x for x in l]
    return out


def pack(scene, cap=None, ccap=None, klcap=None, lcap=None, seed=0):
    """The scene as the arrays of msl.h (a dict keyed by the argument names) and its shape (a dict).  The table rows are random bytes."""
    from manhattanslam_amd import mappoint
    rng = np.random.default_rng(seed)
    n_tab, frames = len(scene["kf_bad"]), scene["frames"]
    n_pts, n_lines = max(len(scene["pt_bad"]), 1), max(len(scene["ln_bad"]), 1)
    cap = cap or max([len(h) for h in scene["held"]] + [len(f["held"]) for f in frames] + [1])
    klcap = klcap or max([len(h) for h in scene["lheld"]] + [1])
    lcap = lcap or max([len(f["lheld"]) for f in frames] + [1])
    ccap = ccap or max([len(c) for c in scene["conn"]] + [1])
    _, t = mappoint.pack_table([dict(desc=np.zeros((len(h), 32), np.uint8), bad=b) for h, b in zip(scene["held"], scene["kf_bad"])], cap)
    o = mappoint.pack_observations([[(k, 0) for k in obs] for obs in scene["pt_obs"]] or [[]])
    raw = lambda n, w, dt: np.frombuffer(rng.integers(0, 256, n * w * np.dtype(dt).itemsize, dtype=np.uint8).tobytes(), dt).reshape(n, w).copy()
    flags = lambda bad, n: np.array([0 if b else 1 for b in bad] + [0] * (n - len(bad)), np.uint8)
    nobs = lambda v, n: np.array(list(v) + [0] * (n - len(v)), np.int32)
    a = dict(kf_flags=t["kf_flags"], n_kps=t["n_kps"], held_id=_rows(scene["held"], cap), obs_off=o["obs_off"], obs_kf=o["obs_kf"],
             conn=_rows(scene["conn"], ccap), n_conn=np.array([len(c) for c in scene["conn"]], np.int32),
             parent=np.array([-1 if p is None else p for p in scene["parent"]], np.int32),
             pt_flags=flags(scene["pt_bad"], n_pts), pt_nobs=nobs(scene["pt_nobs"], n_pts), pt_xyz=raw(n_pts, 3, np.float32),
             pt_normal=raw(n_pts, 3, np.float32), pt_dist=raw(n_pts, 2, np.float32), pt_desc=raw(n_pts, 32, np.uint8),
             lheld_id=_rows(scene["lheld"], klcap), n_kl=np.array([len(h) for h in scene["lheld"]], np.int32),
             ln_flags=flags(scene["ln_bad"], n_lines), ln_nobs=nobs(scene["ln_nobs"], n_lines), ln_xyz=raw(n_lines, 6, np.float64),
             ln_normal=raw(n_lines, 3, np.float64), ln_dist=raw(n_lines, 2, np.float32), ln_desc=raw(n_lines, 32, np.uint8),
             cur_held=_rows([f["held"] for f in frames], cap), n_cur=np.array([len(f["held"]) for f in frames], np.int32),
             cur_lheld=_rows([f["lheld"] for f in frames], lcap), n_cur_lines=np.array([len(f["lheld"]) for f in frames], np.int32),
             prev_kf=_rows([f.get("prev") or [] for f in frames], n_tab), n_prev=np.array([len(f.get("prev") or []) for f in frames], np.int32))
    return a, dict(n_frames=len(frames), n_tab=n_tab, cap=cap, ccap=ccap, klcap=klcap, lcap=lcap, n_pts=n_pts, n_lines=n_lines,
                   n_obs_total=int(o["obs_off"][-1]))


def model(scene):
    """update_local_map of every frame."""
    return [lm.update_local_map(scene, f) for f in scene["frames"]]


def expected(scene, a, sh, mcap, mlcap, want=None):
    """The arrays the three calls leave in outputs that held FILL, from the model's results."""
    want = want or model(scene)
    F, n_tab, cap, lcap = sh["n_frames"], sh["n_tab"], sh["cap"], sh["lcap"]
    e = dict(votes=np.zeros((F, n_tab), np.int32), local_kf=np.full((F, n_tab), -1, np.int32), n_local_kf=np.zeros(F, np.int32),
             ref_kf=np.full(F, -1, np.int32), cur_cleared=np.zeros((F, cap), np.uint8), status=np.zeros(F, np.uint8))
    for pre, ids, m, nx, dt, fc in (("mp", "local_id", mcap, 3, np.float32, cap), ("ml", "local_line_id", mlcap, 6, np.float64, lcap)):
        e[ids] = np.full((F, m), -1, np.int32)
        e["n_local" if pre == "mp" else "n_local_lines"] = np.zeros(F, np.int32)
        for k, w, d in (("xyz", nx, dt), ("normal", 3, dt), ("dist", 2, np.float32), ("desc", 32, np.uint8)):
            e[pre + "_" + k] = np.frombuffer(bytes([FILL]) * (F * m * w * np.dtype(d).itemsize), d).reshape(F, m, w).copy()
        e[pre + "_flags"] = np.zeros((F, m), np.uint8)
        e["cur_flags" if pre == "mp" else "cur_line_flags"] = np.zeros((F, fc), np.uint8)
    for f, w in enumerate(want):
        kf = w["kf"]
        for k, v in kf["votes"].items():
            e["votes"][f, k] = v
        e["local_kf"][f, :len(kf["local_kf"])] = kf["local_kf"]
        e["n_local_kf"][f] = len(kf["local_kf"])
        e["ref_kf"][f] = -1 if kf["ref_kf"] is None else kf["ref_kf"]
        e["cur_cleared"][f, kf["cleared"]] = 1
        e["status"][f] = kf["status"]
        for pre, tab, ids, cnt, cf, m, name in (("mp", "pt", "local_id", "n_local", "cur_flags", mcap, "points"),
                                                ("ml", "ln", "local_line_id", "n_local_lines", "cur_line_flags", mlcap, "lines")):
            r = w[name]
            n = min(len(r["local"]), m)
            loc = np.array(r["local"][:n], np.int64)
            e[ids][f, :n] = loc
            e[cnt][f] = len(r["local"])
            e[pre + "_flags"][f, :n] = r["flags"][:n]
            e[cf][f, :len(r["cur_flags"])] = r["cur_flags"]
            for k in ("xyz", "normal", "dist", "desc"):
                e[pre + "_" + k][f, :n] = a[tab + "_" + k][loc]
    return e


CANARY, GUARD = 0xC3, 256


class DevArray:
    """An array in device memory between two guards of GUARD canary bytes: a copy of `array`, or `shape` elements of `dtype` holding FILL."""

    def __init__(self, array=None, shape=None, dtype=None):
        import torch
        if array is not None:
            array = np.ascontiguousarray(array)
            shape, dtype = array.shape, array.dtype
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.n = int(np.prod(self.shape)) * self.dtype.itemsize
        buf = np.full(self.n + 2 * GUARD, CANARY, np.uint8)
        buf[GUARD:GUARD + self.n] = FILL if array is None else array.reshape(-1).view(np.uint8)
        self.t = torch.from_numpy(buf).cuda()

    def data_ptr(self):
        return self.t.data_ptr() + GUARD

    def numpy(self):
        return self.t.cpu().numpy()[GUARD:GUARD + self.n].view(self.dtype).reshape(self.shape).copy()

    def intact(self):
        b = self.t.cpu().numpy()
        return bool((b[:GUARD] == CANARY).all() and (b[GUARD + self.n:] == CANARY).all())


def host_filled(shape, dtype):
    return np.frombuffer(bytes([FILL]) * (int(np.prod(shape)) * np.dtype(dtype).itemsize), dtype).reshape(shape).copy()


def device_filled(shape, dtype):
    return DevArray(shape=shape, dtype=dtype)


def run(a, sh, mcap, mlcap, mem=0, handle=None, with_prev=True, keep=None):
    """msl_local_keyframes, then msl_local_points and msl_local_lines on its list: mem = 0 on host arrays, 1 on DevArrays (a handle is
    needed).  The outputs hold FILL before.  Returns every output as a numpy array; keep (a dict) receives the arrays as they were passed."""
    from manhattanslam_amd import localmap
    d = {k: DevArray(v) for k, v in a.items()} if mem else dict(a)
    zeros = device_filled if mem else host_filled
    if not with_prev:
        d["prev_kf"] = d["n_prev"] = None
    F, n_tab = sh["n_frames"], sh["n_tab"]
    out = localmap.keyframes_outputs(F, sh["cap"], n_tab, zeros)
    localmap.local_keyframes(F, sh["cap"], n_tab, sh["n_pts"], sh["n_obs_total"], sh["ccap"], d, out, mem, handle=handle)
    d["local_kf"], d["n_local_kf"] = out["local_kf"], out["n_local_kf"]
    out.update(localmap.local_points(F, n_tab, sh["cap"], sh["n_pts"], mcap, d, localmap.points_outputs(F, sh["cap"], mcap, zeros), mem, handle=handle))
    out.update(localmap.local_lines(F, n_tab, sh["klcap"], sh["lcap"], sh["n_lines"], mlcap, d,
                                    localmap.lines_outputs(F, sh["lcap"], mlcap, zeros), mem, handle=handle))
    if handle is not None:
        handle.sync()
    if keep is not None:
        keep.update(d); keep.update(out)
    return {k: (v.numpy() if mem else v) for k, v in out.items()}


def same(got, want):
    """The keys whose bytes differ."""
    return [k for k in want if got[k].shape != want[k].shape or got[k].tobytes() != want[k].tobytes()]

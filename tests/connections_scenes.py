"""Scenes for msl_connections_apply and msl_fuse_targets: random logs, one hand-built scene per pin of msl.h, their packing into the ABI's
arrays, the arrays the model expects of a call, and the calls in their forms.  A scene is a dict: state (tests/connections_model.py),
weight (rows of n_tab weights, or None), ops, origin, th."""
import numpy as np

from tests import connections_model as cm
from tests.localmap_scenes import FILL, DevArray, device_filled, host_filled, same  # noqa: F401

U, B = cm.UPDATE, cm.KF_BAD
WEIGHTS = (1, 3, 14, 15, 16, 20, 40)                                      # around th = 15, with repeats of a stored weight
RANDOM_SEEDS = range(300)                                             # the logs of the model test and of the GPU test


def scene(state, weight, ops, origin=-1, th=15):
    weight = None if weight is None else np.array(weight, np.int32).reshape(-1, len(state["parent"]))
    return dict(state=state, weight=weight, ops=[tuple(o) for o in ops], origin=origin, th=th)


def graph(n_tab, edges, parent=None, ccap=None, flags=None):
    """A consistent state: symmetric weights edges[(i, j)] = w, every ordered row rebuilt from its whole map, parent as a dict, every
    keyframe live and past its first connection (or `flags`)."""
    s = cm.empty(n_tab, ccap, flags if flags is not None else [cm.LIVE | cm.CONNECTED] * n_tab)
    for (i, j), w in edges.items():
        s["cw"][i][j] = s["cw"][j][i] = w
    for k in range(n_tab):
        cm.store(s, k, cm.rebuilt(s["cw"][k]))
        s["parent"][k] = (parent or {}).get(k, -1)
    return s


def model(sc, **kw):
    return cm.apply(sc["state"], [] if sc["weight"] is None else sc["weight"], sc["ops"], sc["origin"], sc["th"], **kw)


# ---- random logs -------------------------------------------------------------------------------------------------------------------------
def random_log(seed, n_tab=None, n_ops=None):
    """5 to 60 ops on 3 to 14 new keyframes; the weight rows come from a symmetric matrix (so that an AddConnection often repeats the
    stored weight) with some entries redrawn, and name keyframes whether they are bad or not."""
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(3, 15)) if n_tab is None else n_tab
    n_ops = int(rng.integers(5, 61)) if n_ops is None else n_ops
    m = rng.choice((0,) + WEIGHTS, (n, n), p=(0.3,) + (0.1,) * 7)
    m = np.triu(m, 1) + np.triu(m, 1).T
    weight = m.copy()
    redraw = rng.random((n, n)) < 0.15
    weight[redraw] = rng.choice((0,) + WEIGHTS, int(redraw.sum()))
    if seed % 5 == 0:
        weight[int(rng.integers(n))] = 0                                  # an empty row
    flags = [cm.LIVE | (cm.NOT_ERASE if rng.random() < 0.1 else 0) | (0x40 if rng.random() < 0.2 else 0) for _ in range(n)]
    origin = -1 if seed % 7 == 3 else 0
    ops = [(U, int(k), int(k)) for k in rng.permutation(n)[:n_ops // 2] if rng.random() < 0.8]   # most keyframes connect before the culling starts
    while len(ops) < n_ops:
        k = int(rng.integers(n))
        if rng.random() < 0.7:
            ops.append((U, k, k if rng.random() < 0.85 else int(rng.integers(n))))
        else:
            ops.append((B, k))
    return scene(cm.empty(n, flags=flags), weight, ops, origin)


# ---- the pins ------------------------------------------------------------------------------------------------------------------------------
def pin_equal_weight_keeps_a_cut_row():
    """Keyframe 0 is cut at th to [1]; keyframe 1 then sends the weight 0 already stores: row 0 is not rebuilt and stays without 2."""
    return scene(cm.empty(4), [[0, 20, 3, 0], [20, 0, 0, 16]], [(U, 0, 0), (U, 1, 1)], origin=0)


def pin_changed_weight_brings_the_entries_below_th():
    """The same, and then keyframe 1 sends 21: row 0 is rebuilt from its whole map and gains 2 with weight 3."""
    return scene(cm.empty(4), [[0, 20, 3, 0], [20, 0, 0, 16], [21, 0, 0, 16]], [(U, 0, 0), (U, 1, 1), (U, 1, 2)], origin=0)


def pin_no_weight_reaches_th():
    """Equal maxima below th: the lowest index alone (strict > in ascending order)."""
    return scene(cm.empty(5), [[0, 0, 7, 7, 3]], [(U, 0, 0), (U, 4, 0)], origin=0)


def pin_equal_weights_in_a_row():
    """Descending weight, equal weights by descending index; INT32_MAX orders as a weight like any other."""
    return scene(cm.empty(6), [[0, 20, 2 ** 31 - 1, 20, 15, 20], [2 ** 31 - 1, 0, 2 ** 31 - 1, 14, 15, 15]], [(U, 0, 0), (U, 1, 1)], origin=0)


def pin_one_directional_entry_survives():
    """0 holds 2 with weight 3, 2 never held 0: KF_BAD of 2 erases nothing in 0, and the next rebuild of row 0 lists the bad 2."""
    return scene(cm.empty(3), [[0, 20, 3], [25, 0, 0]], [(U, 0, 0), (B, 2), (U, 1, 1)], origin=0)


TREE_EDGES = {(1, 0): 20, (1, 2): 20, (1, 3): 20, (1, 4): 20, (1, 5): 20, (1, 6): 20, (1, 7): 20,
              (2, 0): 10, (3, 0): 30, (6, 0): 30, (4, 3): 50, (7, 3): 40, (7, 4): 40}


def pin_tree_loop():
    """KF_BAD of 1 (parent 0, children 2 .. 7).  3 and 6 link to 0 with 30: the first child, 3, wins; 4 links to 3 alone with 50 and is
    re-parented to it next (a re-parented child is a candidate); 7 links to 3 and 4 with 40 each and its row lists 4 first: 7 goes to 4;
    then 6 and 2 go to 0; 5 links to no candidate and gets the original parent 0."""
    return scene(graph(8, TREE_EDGES, {1: 0, 2: 1, 3: 1, 4: 1, 5: 1, 6: 1, 7: 1}), None, [(B, 1)], origin=0)


def pin_tree_loop_without_a_parent():
    """The same with parent[1] == -1: no candidate, every child is left and gets -1."""
    return scene(graph(8, TREE_EDGES, {2: 1, 3: 1, 4: 1, 5: 1, 6: 1, 7: 1}), None, [(B, 1)], origin=0)


def pin_early_returns():
    """The origin and a keyframe with mbNotErase are kept; a second KF_BAD and an UPDATE of a bad keyframe do nothing; a row that is zero
    but for the keyframe's own entry is empty."""
    flags = [cm.LIVE | cm.CONNECTED] * 5
    flags[3] |= cm.NOT_ERASE
    s = graph(5, {(0, 1): 20, (1, 2): 16, (2, 3): 40, (3, 4): 15, (0, 4): 3}, {1: 0, 2: 1, 3: 2, 4: 3}, flags=flags)
    return scene(s, [[20, 20, 20, 20, 20], [0, 0, 0, 0, 9]], [(B, 0), (B, 3), (B, 2), (B, 2), (U, 2, 0), (U, 4, 1), (U, 4, 0)], origin=0)


def pin_first_connection_once():
    """The first UPDATE of 2 sets its parent, the second does not; the origin never gets one, and its bit 2 stays clear."""
    return scene(cm.empty(4), [[0, 30, 0, 16], [0, 16, 0, 30], [0, 15, 15, 15]], [(U, 2, 0), (U, 2, 1), (U, 0, 2), (U, 0, 2)], origin=0)


def pin_ccap_below_the_lists():
    """ccap = 3 under lists of 6 and 7: the stored rows are cut and n_conn is the full count.  The tree loop reads the stored row: child 7
    of 6 holds the candidate 0, but beyond ccap, so it has no link, is left, and gets the original parent 0 all the same.  Row 7 is
    rebuilt by the erasure with 6 entries: one touched row above ccap."""
    edges = {(0, j): 20 + j for j in range(1, 7)}
    edges.update({(7, j): 30 + j for j in range(1, 6)})
    edges.update({(7, 0): 16, (7, 6): 60, (5, 6): 18})
    s = graph(8, edges, {6: 0, 7: 6, 5: 0, 1: 0, 2: 0, 3: 0, 4: 0}, ccap=3)
    return scene(s, [[0, 0, 0, 50, 0, 0, 0, 0]], [(U, 0, 0), (B, 6)], origin=0)


PINS = [pin_equal_weight_keeps_a_cut_row, pin_changed_weight_brings_the_entries_below_th, pin_no_weight_reaches_th, pin_equal_weights_in_a_row,
        pin_one_directional_entry_survives, pin_tree_loop, pin_tree_loop_without_a_parent, pin_early_returns, pin_first_connection_once,
        pin_ccap_below_the_lists]


def all_scenes():
    """The pins, and the random logs in groups of 50 seeds (a case of the GPU test runs one group)."""
    return [(p.__name__, p) for p in PINS]


def random_groups(size=50):
    seeds = list(RANDOM_SEEDS)
    return [seeds[i:i + size] for i in range(0, len(seeds), size)]


def limits_scene():
    """n_tab = 4096, MSL_CONN_MAX_OPS ops.  Keyframe 1 has 300 children (2 .. 301), each linked to 1; child c links to c - 1 with a weight
    that grows with c, and 301 links to the parent 0 of 1, so the tree loop re-parents 301 first and then chains down to 2.  Rows 600 ..
    4095 are pre-filled with a few links.  Op 0 is an UPDATE of 4095 whose row has 4095 non-zero weights, many equal, some below th; then
    KF_BAD of 1; the rest of the log updates and culls keyframes above 600."""
    n, rng = cm.MAX_TAB, np.random.default_rng(5)
    edges = {(1, 0): 20}
    for c in range(2, 302):
        edges[(c, 1)] = 20 + c % 7
        if c > 2:
            edges[(c, c - 1)] = 100 + c
    edges[(301, 0)] = 17
    for k in range(600, n - 1):
        edges[(k, k + 1)] = int(rng.choice(WEIGHTS))
        edges[(k, 300 + (k * 7) % 250)] = int(rng.choice(WEIGHTS))
    parent = {c: 1 for c in range(2, 302)}
    parent[1] = 0
    parent.update({k: k - 1 for k in range(600, n)})
    s = graph(n, edges, parent)
    weight = np.zeros((4, n), np.int32)
    weight[0] = rng.choice(WEIGHTS, n)
    weight[1, 600:700] = rng.choice(WEIGHTS, 100)
    weight[2, 2000:2040] = 40
    weight[3, 650:660] = 15
    ops = [(U, n - 1, 0), (B, 1)]
    while len(ops) < cm.MAX_OPS:
        k = int(rng.integers(600, n))
        ops.append((U, k, int(rng.integers(1, 4))) if rng.random() < 0.8 else (B, k))
    return scene(s, weight, ops, origin=0)


# ---- packing, the expected arrays, the calls ---------------------------------------------------------------------------------------------
def pack(sc, tcap=None):
    """The scene as the arrays of msl.h (a dict keyed by the argument names) and its shape (a dict)."""
    from manhattanslam_amd import connections
    s = sc["state"]
    n_tab, ccap = s["conn"].shape
    a = {k: np.ascontiguousarray(s[k]) for k in cm.STATE_KEYS}
    a.update(weight=sc["weight"], ops=connections.pack_ops(sc["ops"]))
    return a, dict(n_tab=n_tab, ccap=ccap, n_rows=0 if sc["weight"] is None else len(sc["weight"]), n_ops=len(sc["ops"]),
                   tcap=n_tab if tcap is None else tcap, origin=sc["origin"], th=sc["th"])


def expected(sh, want):
    """The arrays a call leaves, from the model's result."""
    from manhattanslam_amd import connections
    e = {k: np.array(want["state"][k]) for k in connections.INOUT_KEYS}
    out = connections.outputs(sh["n_ops"], sh["tcap"], host_filled)
    out["op_status"][:] = want["op_status"]
    out["touched"][:] = (want["touched"] + [-1] * sh["tcap"])[:sh["tcap"]]
    out["counts"][:] = want["counts"]
    e.update(out)
    return e


def run(a, sh, mem=0, handle=None, keep=None):
    """msl_connections_apply: mem = 0 on copies of the host arrays, 1 on DevArrays (a handle is needed).  The outputs hold FILL before.
    Returns every in-place array and output as a numpy array; keep (a dict) receives the arrays as they were passed."""
    from manhattanslam_amd import connections
    d = {k: None if v is None else DevArray(v) if mem else v.copy() for k, v in a.items()}
    out = connections.outputs(sh["n_ops"], sh["tcap"], device_filled if mem else host_filled)
    connections.apply(sh["n_tab"], sh["ccap"], sh["n_rows"], sh["n_ops"], sh["tcap"], sh["origin"], sh["th"], d, d, out, mem, handle=handle)
    if handle is not None:
        handle.sync()
    if keep is not None:
        keep.update({k: v for k, v in d.items() if v is not None}); keep.update(out)
    got = {k: d[k] for k in connections.INOUT_KEYS}
    got.update(out)
    return {k: (v.numpy() if mem else v) for k, v in got.items()}


def targets_expected(lists, n_items, tcap):
    t = np.full((n_items, tcap), -1, np.int32)
    for f, l in enumerate(lists):
        t[f, :min(len(l), tcap)] = l[:tcap]
    return dict(targets=t, n_targets=np.array([len(l) for l in lists], np.int32))


def run_targets(state, cur, nn, nn2, tcap, mem=0, handle=None, keep=None):
    """msl_fuse_targets on the graph of `state`, in the same forms as run."""
    from manhattanslam_amd import connections
    n_tab, ccap = state["conn"].shape
    a = dict(conn=state["conn"], n_conn=state["n_conn"], kf_flags=state["kf_flags"], cur=np.array(cur, np.int32))
    d = {k: DevArray(v) if mem else np.ascontiguousarray(v).copy() for k, v in a.items()}
    out = connections.targets_outputs(len(cur), tcap, device_filled if mem else host_filled)
    connections.fuse_targets(n_tab, ccap, len(cur), nn, nn2, tcap, d, out, mem, handle=handle)
    if handle is not None:
        handle.sync()
    if keep is not None:
        keep.update(d); keep.update(out)
    return {k: (v.numpy() if mem else v) for k, v in out.items()}


# ---- a small map for the chains ------------------------------------------------------------------------------------------------------------
def chain_map(seed, n_tab=12, cap=48, n_pts=160, th=5):
    """A consistent map -- held_id[k][i] == p exactly where point p observes (k, i) -- whose last keyframe is new: flags == 1, no
    connection yet.  The graph of the others is what the model leaves after an UPDATE of each from its own covisibility.  Returns
    dict(held_id, n_kps, pt_flags, obs (per point [(keyframe, keypoint)], ascending), table (keyframe dicts with held_id), state, th)."""
    from tests import mappoint_model as mm
    rng = np.random.default_rng(seed)
    held, n_kps, obs = np.full((n_tab, cap), -1, np.int32), np.zeros(n_tab, np.int32), []
    for p in range(n_pts):
        ks = sorted(int(k) for k in rng.permutation(n_tab)[:int(rng.integers(1, 7))] if n_kps[k] < cap)
        for k in ks:
            held[k, n_kps[k]] = p
        obs.append([(k, int(n_kps[k])) for k in ks])
        for k in ks:
            n_kps[k] += 1
    pt_flags = np.array([0 if rng.random() < 0.1 else 1 for _ in range(n_pts)], np.uint8)
    table = [dict(held_id=held[k][:n_kps[k]]) for k in range(n_tab)]
    old = list(range(n_tab - 1))
    cov = mm.covisibility(table, obs, pt_flags, old, th=th, ccap=n_tab)
    cov["weight"][:, n_tab - 1] = 0                                      # the new keyframe is not in the graph yet
    state = cm.apply(cm.empty(n_tab), cov["weight"], [(U, k, k) for k in old], 0, th)["state"]
    return dict(held_id=held, n_kps=n_kps, pt_flags=pt_flags, obs=obs, table=table, state=state, th=th, cur=n_tab - 1)

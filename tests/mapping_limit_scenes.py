"""Scenes for the local-map and culling entries at the limits include/msl.h accepts: n_tab 4096, cap 8192, klcap / lcap 256, mcap / mlcap
32768, n_items 4096, n_pts 1 << 20 and n of msl_cull_recent 1 << 20.  One builder per case, a to k; each returns the scene (the dict of
tests/localmap_model.py or tests/cull_model.py, built with the helpers of tests/localmap_scenes.py and tests/cull_scenes.py) together with
the facts it was built to reach.  tests/test_mapping_limit_scenes.py asserts those facts on the sequential models without a GPU;
tests/test_mapping_limits_gpu.py runs the entries on the same scenes.  The builders, their models and their packed arrays are computed once
per process (case, want_localmap, want_cull, packed) and must be left as they are; the functions after `pack` that touch the packed arrays
(absent ids, NaN payloads, the padding to a million points) work on copies."""
import functools

import numpy as np

from tests import cull_model as cm
from tests import cull_scenes as cs
from tests import localmap_model as lm
from tests import localmap_scenes as ls

MAX_TAB, MAX_CAP, MAX_KLCAP, MAX_MCAP, MAX_ITEMS, MAX_PTS, MAX_RECENT = 4096, 8192, 256, 32768, 4096, 1 << 20, 1 << 20
LKF_NT, LM_NT, WAVE = 1024, 256, 64                                   # k_local_kf's / k_cull_kf's workgroup, the k_lm_* kernels', a wave


def kept_slots(local_kf, kf_held, bad):
    """Per list position the slots whose element enters the local list: live, and met for the first time in list order.  An entry outside
    the table keeps nothing."""
    seen, out = set(), []
    for k in local_kf:
        row = []
        if 0 <= k < len(kf_held):
            for i, p in enumerate(kf_held[k]):
                if p is not None and not bad[p] and p not in seen:
                    seen.add(p)
                    row.append(i)
        out.append(row)
    return out


def _new_point(s, rng, bad=False, observers=()):
    """A point no keyframe holds yet; Observations() is 0, 1 or 2."""
    s["pt_bad"].append(bad); s["pt_obs"].append(list(observers)); s["pt_nobs"].append(int(rng.integers(0, 3)))
    return len(s["pt_bad"]) - 1


# ---- a to c: msl_local_keyframes -------------------------------------------------------------------------------------------------------
def lkf_every_keyframe_voted():
    """a. n_tab 4096, cap 8.  Frame 0: both of its points are observed by every keyframe, so all 4096 get the same vote.  Frame 1: one
    more vote for 4095.  Frame 2: no votes and a prev_kf row of 4096 entries."""
    n = MAX_TAB
    s = ls.graph(n)
    everyone = [ls.add_point(s, range(n)) for _ in range(2)]
    top = ls.add_point(s, [n - 1])
    prev = [int(k) for k in np.random.default_rng(1).permutation(n)]
    s["frames"] = [dict(held=everyone * 4, lheld=[], prev=[]), dict(held=everyone * 3 + [None, top], lheld=[], prev=[]),
                   dict(held=[None, None], lheld=[], prev=prev)]
    return s, dict(n_tab=n, cap=8, lists=[list(range(n)), list(range(n)), prev], ref=[0, n - 1, None], votes0=[8] * n)


def lkf_walk_over_the_whole_table():
    """b. n_tab = ccap = 4096, 68 voted keyframes from 0 to 4095, three frames over one graph.
    Keyframe 0: n_conn = ccap, its ten best are nine listed keyframes and 4040; children 1000 (bad), 2081 (voted), 2085, 3000.
    Keyframe 68: n_conn 11, the ten best all listed and the eleventh not; its only child is 4095.
    Keyframe 129: neighbours 1000 (bad), 68, 4041; parent 4095.  Ten more voted keyframes have a bad and a free neighbour.
    Frame 0 votes for all 68, frame 1 for all but 4095, frame 2 for all but 4095 and 68."""
    n = MAX_TAB
    voted = sorted({0, n - 1} | {61 * k + 7 for k in range(1, 67)})
    assert len(voted) == 68 and {68, 129, 2081} <= set(voted) and not {1000, 2085, 3000, 3001, 4040, 4041} & set(voted)
    conn = {0: voted[1:10] + [4040] + [(7 * i + 1) % n for i in range(n - 10)],
            68: [k for k in voted[:12] if k != 68][:10] + [3001],
            129: [1000, 68, 4041]}
    for j, k in enumerate(voted[10:20]):
        conn[k] = [1000, 4042 + j]
    parent = {1000: 0, 2081: 0, 2085: 0, 3000: 0, n - 1: 68, 129: n - 1}
    s = ls.graph(n, conn=conn, parent=parent, kf_bad=(1000,))
    point = {k: ls.add_point(s, [k]) for k in voted}
    for without in ((), (n - 1,), (n - 1, 68)):
        held = [point[k] for k in voted if k not in without for _ in range(1 + k % 3)]
        s["frames"].append(dict(held=held, lheld=[], prev=[]))
    return s, dict(n_tab=n, ccap=n, voted=voted, neighbour=4040, middle_child=2085, skipped_children=(1000, 2081), later_child=3000,
                   childless=68, top=n - 1, eleventh=3001)


def lkf_full_frame():
    """c. cap 8192, n_tab 6.  Frame 0 holds 8192 slots, frames 1 and 2 its first 1025 and 1024.  Every live point is observed by keyframe
    2, sixteen of them twice (two observations, two votes); bad points sit in slots 1024, 1025, 5000 and 8191."""
    n_tab, cap = 6, MAX_CAP
    s = ls.graph(n_tab, kf_bad=(4,))
    live = [ls.add_point(s, [2, 2, 3] if p < 16 else [2] + ([p % n_tab] if p % n_tab != 2 else [])) for p in range(500)]
    dead = [ls.add_point(s, [1], bad=True) for _ in range(3)]
    held = [live[i % 500] for i in range(cap)]
    held[5] = held[3000] = None
    bad_slots = {1024: dead[0], 1025: dead[1], 5000: dead[2], cap - 1: dead[0]}
    for i, p in bad_slots.items():
        held[i] = p
    s["frames"] = [dict(held=held[:m], lheld=[], prev=[]) for m in (cap, LKF_NT + 1, LKF_NT)]
    return s, dict(n_tab=n_tab, cap=cap, n_cur=[cap, LKF_NT + 1, LKF_NT], cleared=[sorted(bad_slots), [1024], []], voted=2)


# ---- d to h: msl_local_points / msl_local_lines ------------------------------------------------------------------------------------------
CUT_SLOT = 5 * LM_NT + 100                                            # d: the output capacity ends inside the sixth chunk of the full row


def points_full_keyframe():
    """d. cap 8192, n_tab 5: keyframes of 257, 8192, 256, 0 and 300 slots, all in the list.  In the full row every chunk of 256 slots but
    the eighth keeps something, the first and the last slot among them; the eighth holds NULLs, bad points and ids met before.  The frame
    holds 8192 ids; its last block has live, bad, NULL and repeated ones."""
    rng = np.random.default_rng(4)
    n_tab, cap = 5, MAX_CAP
    s = ls.graph(n_tab)
    voter = _new_point(s, rng, observers=range(n_tab))
    dead = [_new_point(s, rng, bad=True) for _ in range(20)]
    first = [_new_point(s, rng) for _ in range(250)]
    s["held"][0] = [first[i] for i in rng.permutation(250)] + dead[:4] + [None] * 3
    rng.shuffle(s["held"][0])
    known = list(first)

    def stale():
        r = rng.random()
        return None if r < 0.25 else dead[int(rng.integers(0, 20))] if r < 0.5 else known[int(rng.integers(0, len(known)))]

    def row(n, fresh, pinned=(), nothing=()):
        out = []
        for i in range(n):
            p = _new_point(s, rng) if i in pinned or (i // LM_NT not in nothing and rng.random() < fresh) else stale()
            out.append(p)
            if p is not None and not s["pt_bad"][p]:
                known.append(p)
        return out

    s["held"][1] = row(cap, 0.55, pinned=(0, cap - 1), nothing=(7,))
    s["held"][2] = row(LM_NT, 0.3)
    s["held"][4] = row(300, 0.3)
    cur = [voter] + [stale() for _ in range(cap - 1)]
    cur[cap - LM_NT:cap - LM_NT + 5] = [known[100], dead[0], None, known[200], known[200]]
    cur[cap - 1] = known[-1]
    s["frames"] = [dict(held=cur, lheld=[], prev=[])]
    return s, dict(n_tab=n_tab, cap=cap, n_kps=[LM_NT + 1, cap, LM_NT, 0, 300], empty_chunk=7, full=1, cut_slot=CUT_SLOT,
                   last_block=(cap - LM_NT, cap))


def mcap_cut():
    """d: the count of outputs up to CUT_SLOT of the full keyframe -- an output capacity that ends inside its sixth chunk."""
    s, facts = case("d")
    kept = kept_slots(want("d")[0]["kf"]["local_kf"], s["held"], s["pt_bad"])
    return sum(len(r) for r in kept[:facts["full"]]) + sum(1 for i in kept[facts["full"]] if i < CUT_SLOT)


def points_full_list():
    """e. A list of 4096 entries (n_tab 4096, cap 4), handed over as prev_kf of a frame without votes so that it can be any list: a
    permutation of the table in which position 300 names a keyframe that holds nothing (the GPU test replaces it by an index outside the
    table) and position 2000 names the keyframe of position 10 again.  Keyframes hold 0 to 4 slots of a pool with repeats; those at
    positions 255, 256, 257 and 4095 start with a point nobody else holds."""
    rng = np.random.default_rng(5)
    n, cap = MAX_TAB, 4
    s = ls.graph(n)
    pool = [_new_point(s, rng, bad=bool(rng.random() < 0.1)) for _ in range(3000)]
    for k in range(n):
        s["held"][k] = [None if rng.random() < 0.15 else pool[int(rng.integers(0, 3000))] for _ in range(int(rng.integers(0, cap + 1)))]
    order = [int(k) for k in rng.permutation(n)]
    for pos in (LM_NT - 1, LM_NT, LM_NT + 1, n - 1):
        s["held"][order[pos]] = [_new_point(s, rng)] + s["held"][order[pos]][:cap - 1]
    s["held"][order[300]] = []
    order[2000] = order[10]
    s["frames"] = [dict(held=[], lheld=[], prev=order)]
    return s, dict(n_tab=n, cap=cap, absent_pos=300, twice=(10, 2000), scan_positions=(LM_NT - 1, LM_NT, LM_NT + 1, n - 1))


def points_output_capacity(extra=0):
    """f. n_tab 64, cap 600: every keyframe holds 512 live points of its own, 44 NULLs and 44 bad ones, so n_local is 32768 = mcap; with
    extra = 1 the last keyframe holds one live point more."""
    rng = np.random.default_rng(6)
    n_tab, cap, per = 64, 600, 512
    s = ls.graph(n_tab)
    voter = _new_point(s, rng, observers=range(n_tab))
    dead = [_new_point(s, rng, bad=True) for _ in range(8)]
    for k in range(n_tab):
        slots = [_new_point(s, rng) for _ in range(per)] + [None] * 44 + [dead[i % 8] for i in range(44)]
        s["held"][k] = [slots[i] for i in rng.permutation(cap)]
    if extra:
        s["held"][n_tab - 1][max(i for i, p in enumerate(s["held"][n_tab - 1]) if p is None)] = _new_point(s, rng)
    s["frames"] = [dict(held=[voter, s["held"][0][0], s["held"][n_tab - 1][cap - 1], dead[0]], lheld=[], prev=[])]
    return s, dict(n_tab=n_tab, cap=cap, n_local=n_tab * per + extra)


def points_output_capacity_plus_one():
    return points_output_capacity(1)


NAN_WORDS = np.array([0x7FF8000000000123, 0xFFF0000000000001, 0x8000000000000000, 0x7FF0000000000000], np.uint64)   # two NaNs, -0.0, +inf


def lines_full_rows():
    """g. klcap = lcap = 256 with every row full, n_tab 8, 1500 lines: more than 256 local lines, found again in later keyframes."""
    rng = np.random.default_rng(7)
    n_tab, n_lines = 8, 1500
    s = ls.graph(n_tab)
    voter = _new_point(s, rng, observers=range(n_tab))
    s["ln_bad"] = [bool(rng.random() < 0.1) for _ in range(n_lines)]
    s["ln_nobs"] = [int(rng.integers(0, 3)) for _ in range(n_lines)]
    line = lambda: None if rng.random() < 0.05 else int(rng.integers(0, n_lines))
    s["lheld"] = [[line() for _ in range(MAX_KLCAP)] for _ in range(n_tab)]
    s["frames"] = [dict(held=[voter], lheld=[line() for _ in range(MAX_KLCAP)], prev=[])]
    return s, dict(n_tab=n_tab, klcap=MAX_KLCAP, lcap=MAX_KLCAP)


def line_payloads(a, local):
    """NaN, negative-zero and infinity words in ln_xyz and ln_normal of the first, a middle and the last local line (a: packed, changed in
    place before `expected` reads it)."""
    for r, p in enumerate((local[0], local[len(local) // 2], local[-1])):
        a["ln_xyz"].view(np.uint64)[p, r:r + 4] = NAN_WORDS
        a["ln_normal"].view(np.uint64)[p, :3] = NAN_WORDS[r:r + 3] if r < 2 else NAN_WORDS[:3]
    return a


def points_table_small():
    """h. A random scene of 200 points in which ids 0 and 199 are live, held by every keyframe with two slots or more and by every frame;
    pad_points moves id 199 to (1 << 20) - 1."""
    s = ls.random_scene(8, n_tab=20, cap=30, n_pts=200, frame_sizes=[30, 10, 25], klcap=3, lcap=3)
    s["pt_bad"][0] = s["pt_bad"][199] = False
    for row in s["held"] + [f["held"] for f in s["frames"]]:
        if len(row) >= 2:
            row[0], row[1] = 0, 199
    return s, dict(first=0, last=199, n_frames=3)


def absent_ids(a, sh):
    """A copy of the packed arrays in which the NULL slots of held_id and cur_held name ids outside the point table (device memory only)."""
    a = dict(a, held_id=a["held_id"].copy(), cur_held=a["cur_held"].copy())
    a["held_id"][a["held_id"] == -1] = np.resize([sh["n_pts"], -7, 1 << 30], (a["held_id"] == -1).sum())
    a["cur_held"][a["cur_held"] == -1] = np.resize([sh["n_pts"], -5, 1 << 30], (a["cur_held"] == -1).sum())
    return a


def pad_points(a, sh, e, n_pts=MAX_PTS):
    """The packed scene with its point table padded to n_pts rows (the scene's rows, tiled; all live) and its last id moved to n_pts - 1:
    copies of a, sh and of the expectation e with that id renamed.  The observations of the moved id are the last of the table, so obs_off
    stays ascending."""
    small, last, top = sh["n_pts"], sh["n_pts"] - 1, n_pts - 1
    a, e = dict(a), dict(e)
    for k in ("pt_flags", "pt_nobs", "pt_xyz", "pt_normal", "pt_dist", "pt_desc"):
        big = np.resize(a[k], (n_pts,) + a[k].shape[1:])
        big[top] = a[k][last]
        a[k] = big
    a["pt_flags"][last] = 0                                               # nobody names it any more
    off = np.full(n_pts + 1, a["obs_off"][last], np.int32)
    off[:small] = a["obs_off"][:small]
    off[n_pts] = a["obs_off"][small]
    a["obs_off"] = off
    for k in ("held_id", "cur_held"):
        a[k] = np.where(a[k] == last, top, a[k]).astype(np.int32)
    e["local_id"] = np.where(e["local_id"] == last, top, e["local_id"]).astype(np.int32)
    return a, dict(sh, n_pts=n_pts), e


# ---- i, j: msl_cull_keyframes ----------------------------------------------------------------------------------------------------------
def cull_whole_table():
    """i. n_tab = ccap = n_items = 4096, cap 8.  Item 0 walks the whole table: first the keyframes 5, 2023 and 4095 (bitmap words 0, 63
    and 127), each redundant through three keyframes that are not; then everyone else in a random order; last the keyframes 40, 2100 and
    4000, each of which shares two points with its early keyframe that are redundant only while it stands, and two weak points that turn
    bad with it.  4070 is the origin; 4080 is redundant and mbNotErase.  The other keyframes hold points observed twice or four to seven times
    inside a window of seventeen keyframes and cull each other in chains.  Items 1 .. 4095 have two candidates (twenty more every 64th):
    the late keyframe after its early one, or after another keyframe."""
    rng = np.random.default_rng(9)
    n, cap = MAX_TAB, 8
    s = cs.graph(n, origin=4070)
    early, late, held_back = [5, 63 * 32 + 7, n - 1], [40, 2100, 4000], 4080
    spare = iter(range(3000, 3100))
    reserved = set(early + late + [held_back]) | set(range(3000, 3100))
    quiet = lambda: [(next(spare), 0, True) for _ in range(3)]            # octave 0: nothing at octave 2 is redundant for them
    for a, b in zip(early, late):
        h, u = quiet(), quiet()
        for _ in range(4):
            cs.add_point(s, [(a, 2, True)] + h)
        for _ in range(2):
            cs.add_point(s, [(a, 2, True), (b, 2, True)] + u[:2])
        for _ in range(2):                                                # Observations() 3: a's stereo erasure leaves 1
            p = cs.add_point(s, [(a, 2, True), (b, 2, False)])
            s["depth"][a][s["pt_obs"][p][0][1]] = 50.0                    # beyond mThDepth for a: not among its n_mps
        for _ in range(3):
            cs.add_point(s, [(b, 2, True)] + u)
    h = quiet()
    for _ in range(cap):
        cs.add_point(s, [(held_back, 2, True)] + h)
    s["not_erase"][held_back] = True
    for _ in range(4500):
        c = int(rng.integers(0, n))
        window = [k for k in range(max(0, c - 8), min(n, c + 9)) if k not in reserved and len(s["held"][k]) < cap]
        if len(window) >= 4:
            obs = rng.permutation(window)[:2 if rng.random() < 0.15 else int(rng.integers(4, 8))]   # two observers: bad at the first erasure
            p = cs.add_point(s, [(int(k), int(rng.choice([0, 1, 1, 2])), bool(rng.random() < 0.6)) for k in obs], bad=bool(rng.random() < 0.03))
            if len(obs) == 2:                                             # too deep for its first observer, which can so be culled
                s["depth"][int(obs[0])][s["pt_obs"][p][0][1]] = 50.0
    rest = [int(k) for k in rng.permutation(n) if k not in early and k not in late]
    s["items"] = [early + rest + late]
    for f in range(1, MAX_ITEMS):
        j = f % 3
        item = [early[j] if f % 2 else f, late[j]]
        if f % 64 == 0:
            item += [int(k) for k in rng.permutation(n) if k not in item][:20]
        s["items"].append(item)
    return s, dict(n_tab=n, cap=cap, ccap=n, n_items=MAX_ITEMS, early=early, late=late, origin=4070, held_back=held_back,
                   late_entry=(7, 5, 0, cm.KEPT), late_after=(5, 3, 2, cm.KEPT))


def cull_full_keyframes():
    """j. cap 8192, n_tab 6: slot i of every keyframe holds point i, observed by all six in stereo, with these exceptions.  Candidate c
    (keyframes 0 .. 3) holds the points of its own set N[c] at octave 0 and the rest at octave 3; the keyframes 4 and 5 hold everything at
    octave 0: a point of N[c] has two qualifying observers for c, every other point at least three.  |N| = 820, 809, 819, 400.
    In the ten slots G the keyframes 1 and 3 hold a weak point of their own (1 in stereo, 3 in mono, Observations() 3).  Keyframe 5 does not
    hold the hundred points M.  One slot of keyframe 2 lies beyond mThDepth.  Keyframe 1 holds the points ja and jb (both above 1024) in each
    other's slot while their observations name their own, ja's at a mono keypoint.
    Item 0 = [0, 1, 2, 3]: 7372 of 8192 is kept, 7373 of 8192 culled, 7372 of 8191 culled; keyframe 3 then loses the ten weak points, and
    the points of M have only two observers left."""
    rng = np.random.default_rng(10)
    C, n_tab = MAX_CAP, 6
    ids = [int(i) for i in rng.permutation(C)]
    N = [set(ids[0:820]), set(ids[820:1629]), set(ids[1629:2448]), set(ids[2448:2848])]
    M, G, deep = set(ids[2848:2948]), ids[2948:2958], ids[2958]
    ja, jb = [i for i in ids[2959:] if i > LKF_NT][:2]
    s = cs.graph(n_tab)
    s["pt_bad"], s["pt_obs"], s["pt_nobs"] = [False] * (C + 10), [[] for _ in range(C + 10)], [0] * (C + 10)
    for k in range(n_tab):
        for i in range(C):
            p = C + G.index(i) if k in (1, 3) and i in G else None if k == 5 and i in M else i
            stereo = not (k == 3 and i in G) and not (k == 1 and i == ja)
            cs.add_slot(s, k, p, octave=0 if k > 3 or i in N[k] else 3, stereo=stereo, depth=50.0 if (k, i) == (2, deep) else 1.0)
            if p is not None:
                s["pt_obs"][p].append((k, i))
                s["pt_nobs"][p] += 2 if stereo else 1
    s["held"][1][ja], s["held"][1][jb] = jb, ja
    s["items"] = [[0, 1, 2, 3], [3, 0], [1, 3]]
    rows = [(C, 7372, 0, cm.KEPT), (C, 7373, 0, cm.CULLED), (C - 1, 7372, 0, cm.CULLED), (C - 10, C - 10 - 500, 10, cm.CULLED)]
    return s, dict(n_tab=n_tab, cap=C, rows=rows, not_redundant=N, swapped=(ja, jb), weak=G)


# ---- k: msl_cull_recent ----------------------------------------------------------------------------------------------------------------
def recent_tiled(n, th_obs, form, host=False):
    """The 320 elements of tests/test_cull_gpu.py tiled to n, and the verdicts of the tiled model.  host: without the elements the host
    check refuses in the integer form (visible == 0)."""
    from tests.test_cull_gpu import ELEMENTS, recent_arrays, recent_model
    small = recent_arrays(ELEMENTS)
    want = recent_model(small, th_obs, form)
    if host:
        ok = want != cm.RECENT_INVALID
        small, want = {k: v[ok] for k, v in small.items()}, want[ok]
    return {k: np.resize(v, n) for k, v in small.items()}, np.resize(want, n)


# ---- built once ------------------------------------------------------------------------------------------------------------------------
LOCALMAP_CASES = dict(a=lkf_every_keyframe_voted, b=lkf_walk_over_the_whole_table, c=lkf_full_frame, d=points_full_keyframe, e=points_full_list,
                      f=points_output_capacity, f1=points_output_capacity_plus_one, g=lines_full_rows, h=points_table_small)
CULL_CASES = dict(i=cull_whole_table, j=cull_full_keyframes)
PACK = dict(a=dict(cap=8), b=dict(ccap=MAX_TAB), c=dict(cap=MAX_CAP), d=dict(cap=MAX_CAP), e=dict(cap=4), f=dict(cap=600), f1=dict(cap=600),
            g=dict(klcap=MAX_KLCAP, lcap=MAX_KLCAP), h=dict(cap=30), i=dict(cap=8, ccap=MAX_TAB), j=dict(cap=MAX_CAP, ccap=4))


@functools.lru_cache(maxsize=None)
def case(name):
    """(scene, facts) of case `name`."""
    return (LOCALMAP_CASES.get(name) or CULL_CASES[name])()


@functools.lru_cache(maxsize=None)
def want(name):
    """The sequential model's results for case `name`: localmap_scenes.model or cull_scenes.model."""
    return (ls if name in LOCALMAP_CASES else cs).model(case(name)[0])


@functools.lru_cache(maxsize=None)
def packed(name):
    """(a, sh) of case `name` from localmap_scenes.pack or cull_scenes.pack."""
    return (ls if name in LOCALMAP_CASES else cs).pack(case(name)[0], **PACK[name])

"""msl_cull_keyframes and msl_cull_recent on the GPU against tests/cull_model.py: every output, compared as bytes, in the host-memory forms
(the handle's and the device-indexed one) and the device-memory form; every pin on a hand-built scene; the device-memory contract for
indices outside their tables with canaries around every array; and the chain msl_covisibility -> msl_cull_keyframes on one stream in
device memory against both models.  The shapes here are small (n_tab up to 70, cap up to 1100, three items, 320 recent elements); the limits
of msl.h -- n_tab = ccap = n_items 4096, cap 8192, 1 << 20 recent elements -- are in tests/test_mapping_limits_gpu.py."""
import itertools

import numpy as np
import pytest

from tests import cull_model as cm
from tests import cull_scenes as cs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher():
    from manhattanslam_amd.match import Matcher
    h = Matcher()
    yield h
    h.close()


def check(scene, matcher, forms=("device", "host"), **shape):
    """Every output equals the array model's, in each form; returns the model's results."""
    a, sh = cs.pack(scene, **shape)
    want = cs.model(scene)
    e = cs.expected(sh, want)
    for form in forms:
        got = cs.run(a, sh, mem=form == "device", handle=None if form == "batch" else matcher)
        assert cs.same(got, e) == [], (form, {k: (got[k].tolist(), e[k].tolist()) for k in cs.same(got, e)} if sh["n_tab"] < 10 else cs.same(got, e))
    return want


# (6, 1100): more slots than one round of the kernel's workgroup of 1024; (40, 300): more than one round of a workgroup of 256
@pytest.mark.parametrize("n_tab,cap", [(3, 5), (70, 100), (40, 300), (6, 1100)])
def test_random_graphs_in_every_form(matcher, n_tab, cap):
    s = cs.random_scene(n_tab + cap, n_tab, cap, n_items=3)
    want = check(s, matcher, forms=("device", "host", "batch"))
    if n_tab >= 40:
        assert max(len(order) for _, order in want) >= 3                   # a chain of culls
        for c, (rows, order) in zip(s["items"], want):
            assert cm.cull_keyframes_literal(s, c)[:2] == (rows, order)


@pytest.mark.parametrize("pin", cs.PINS, ids=lambda p: p.__name__)
def test_hand_built_scenes(matcher, pin):
    s, rows = pin()
    want = check(s, matcher)
    assert [w[0] for w in want] == rows


def test_indices_outside_their_tables_are_absent_and_nothing_is_written_outside(matcher):
    """The device-memory contract: an out-of-table cand, obs_kf, obs_idx, held_id and origin and counts beyond their capacity give the
    result of the scene without them, and the canaries around every input and output stay."""
    n_tab, cap = 30, 40
    s = cs.random_scene(5, n_tab, cap, n_items=3)
    s["origin"] = None
    full = max(range(n_tab), key=lambda k: len(s["held"][k]))
    s["items"][0] = [int(k) for k in np.random.default_rng(1).permutation(n_tab)]       # a full row: n_cand above ccap is clamped
    s["items"][1] = s["items"][1][:3] + [n_tab, -1, 1 << 30] + s["items"][1][3:12]     # absent candidates in the middle of the walk
    want = cs.model(s)
    assert sum(len(order) for _, order in want) >= 6 and [r[3] for r in want[1][0][3:6]] == [cm.ABSENT] * 3
    ghost = dict(s, pt_obs=[list(o) + [(0, 0)] for o in s["pt_obs"]])                   # one more observation per point, made absent below
    a, sh = cs.pack(ghost)
    assert sh["cap"] == len(s["held"][full]) and sh["ccap"] == n_tab
    e = cs.expected(sh, want)
    last = a["obs_off"][1:] - 1
    a["obs_kf"][last[0::2]] = np.resize([n_tab, -3, 1 << 30], len(last[0::2]))
    a["obs_kf"][last[1::2]] = np.arange(len(last[1::2])) % n_tab                        # a keyframe of the table, the keypoint outside it
    a["obs_idx"][last[1::2]] = np.resize([sh["cap"], -1, 1 << 30], len(last[1::2]))
    a["held_id"][a["held_id"] == -1] = np.resize([sh["n_pts"], -7, 1 << 30], (a["held_id"] == -1).sum())
    a["n_cand"][0] = n_tab + 5; a["n_kps"][full] = sh["cap"] + 1                        # full rows: the clamp changes nothing
    for origin in (n_tab + 3, -5):
        keep = {}
        got = cs.run(a, dict(sh, origin=origin), mem=1, handle=matcher, keep=keep)
        assert cs.same(got, e) == []
        assert [k for k, v in keep.items() if not v.intact()] == []


def test_chain_from_covisibility_on_one_stream_in_device_memory(matcher):
    """msl_covisibility for every keyframe, its conn / n_conn rows passed straight on as cand / n_cand with nothing read back in between:
    one item per keyframe, against the array model and the literal one."""
    from manhattanslam_amd import cull, mappoint
    from tests import mappoint_model as mm
    n_tab, cap, th = 24, 30, 4
    s = cs.random_scene(77, n_tab, cap, n_items=1)
    a, sh = cs.pack(dict(s, items=[[] for _ in range(n_tab)]), ccap=n_tab)
    cv = mm.covisibility([dict(held_id=r[:n]) for r, n in zip(a["held_id"], a["n_kps"])], s["pt_obs"], a["pt_flags"], list(range(n_tab)), th=th, ccap=n_tab)
    s["items"] = [[int(c) for c in cv["conn"][k, :cv["n_conn"][k]]] for k in range(n_tab)]
    want = cs.model(s)
    assert sum(len(order) > 1 for _, order in want) > n_tab // 2 and max(len(c) for c in s["items"]) > 8
    for c, (rows, order) in zip(s["items"], want):
        assert cm.cull_keyframes_literal(s, c)[:2] == (rows, order)
    D = cs.DevArray
    d = {k: D(v) for k, v in a.items()}
    covis = {k: D(v) for k, v in mappoint.covisibility_outputs(n_tab, n_tab, n_tab).items()}
    mappoint.covisibility_device(matcher, n_tab, sh["cap"], sh["n_pts"], n_tab, sh["n_obs_total"], n_tab, th, d["held_id"], d["n_kps"], d["pt_flags"],
                                 d["obs_off"], d["obs_kf"], D(np.arange(n_tab, dtype=np.int32)), covis)
    d["cand"], d["n_cand"] = covis["conn"], covis["n_conn"]
    out = cull.cull_keyframes_device(matcher, cull.cull_params(sh["th_depth"]), n_tab, sh["cap"], sh["n_pts"], n_tab, sh["n_obs_total"], n_tab,
                                     sh["origin"], d, cull.keyframes_outputs(n_tab, n_tab, cs.device_filled))
    matcher.sync()
    assert np.array_equal(covis["conn"].numpy(), cv["conn"]) and np.array_equal(covis["n_conn"].numpy(), cv["n_conn"])
    assert cs.same({k: v.numpy() for k, v in out.items()}, cs.expected(dict(sh, n_items=n_tab), want)) == []
    assert all(v.intact() for v in list(d.values()) + list(out.values()))


# ---- the recent elements -------------------------------------------------------------------------------------------------------------------
CUR = 40
ELEMENTS = list(itertools.product((1, 0), ((0, 0), (4, 0), (1, 3), (1, 4), (1, 5), (3, 4), (0, 7), (9, 2)), (0, 1, 2, 3, 4), (1, 2, 3, 4)))


def recent_arrays(elements):
    live, ratio, age, nobs = zip(*elements)
    return dict(found=np.array([r[0] for r in ratio], np.int32), visible=np.array([r[1] for r in ratio], np.int32),
                first_kf_id=np.array([CUR - x for x in age], np.int32), nobs=np.array(nobs, np.int32), flags=np.array(live, np.uint8) | 4)


def recent_model(a, th_obs, form):
    return np.array([cm.cull_recent(int(f), int(v), int(k), int(n), bool(fl & 1), CUR, th_obs, form)
                     for f, v, k, n, fl in zip(a["found"], a["visible"], a["first_kf_id"], a["nobs"], a["flags"])], np.uint8)


@pytest.mark.parametrize("form", [cm.RATIO_FLOAT, cm.RATIO_INT])
@pytest.mark.parametrize("th_obs", [3, 2])
def test_recent_elements_every_branch(matcher, form, th_obs):
    from manhattanslam_amd import cull
    a = recent_arrays(ELEMENTS)
    n, want = len(ELEMENTS), recent_model(recent_arrays(ELEMENTS), th_obs, form)
    assert set(want.tolist()) == set(range(5)) | ({cm.RECENT_INVALID} if form == cm.RATIO_INT else set()) and n > 257
    d = {k: cs.DevArray(v) for k, v in a.items()}
    for m in (n, 1, 257):                                                  # one element, and one more than a workgroup
        v = cull.cull_recent_device(matcher, m, CUR, th_obs, form, d, cs.device_filled((n,), np.uint8))
        matcher.sync()
        assert np.array_equal(v.numpy()[:m], want[:m]) and (v.numpy()[m:] == cs.FILL).all() and v.intact()
    assert all(x.intact() for x in d.values())
    # host memory refuses the integer form's division by zero, so those elements stay out
    ok = [e for e, w in zip(ELEMENTS, want) if w != cm.RECENT_INVALID]
    h = recent_arrays(ok)
    for handle in (matcher, None):
        v = cull.cull_recent(len(ok), CUR, th_obs, form, h, cs.host_filled((len(ok),), np.uint8), handle=handle)
        assert np.array_equal(v, recent_model(h, th_obs, form))


def test_ratio_forms_differ_on_one_of_three(matcher):
    from manhattanslam_amd import cull
    a = recent_arrays([(1, (1, 3), 1, 9)])
    got = [int(cull.cull_recent(1, CUR, 3, form, a, np.zeros(1, np.uint8), handle=matcher)[0]) for form in (cm.RATIO_FLOAT, cm.RATIO_INT)]
    assert got == [cm.RECENT_KEEP, cm.RECENT_CULL_RATIO]

"""The two sequential models of LocalMapping::KeyFrameCulling in tests/cull_model.py agree: the array model msl_cull_keyframes is compared
with, which carries only the set of culled keyframes from candidate to candidate, and the literal one with objects, EraseMapPointMatch and
SetBadFlag.  Every hand-built scene gives the rows written beside it, and scenes 1 to 11 tell the right model from one that reads only the
entry state or assumes consistent tables.  The two ratio forms of the recent-element cullings differ where the reference's do.  No GPU."""
import numpy as np
import pytest

from tests import cull_model as cm
from tests import cull_scenes as cs

SHAPES = [(3, 5), (8, 12), (12, 20), (20, 30), (30, 16)]


def test_array_model_equals_literal_model_on_random_graphs():
    scenes = [cs.random_scene(seed, *SHAPES[seed % len(SHAPES)], n_items=3) for seed in range(60)]
    with_cull = mono = stereo = unobserved = unheld = gone = not_erase = 0
    for s in scenes:
        culls = 0
        for c in s["items"]:
            rows, order = cm.cull_keyframes(s, c)
            lrows, lorder, lstate = cm.cull_keyframes_literal(s, c)
            assert rows == lrows and order == lorder                           # every counter and status
            assert cm.replay(s, order) == lstate                              # badness, nObs and observation sets after the caller's replay
            state = cm.final_state(s, order)                                  # and by the array model's own rules (nObs of live points)
            assert [(b, None if b else n, o) for b, n, o in lstate] == state
            culls += len(order)
            gone += sum(r[2] for r in rows); not_erase += sum(r[3] == cm.NOT_ERASE for r in rows)
        with_cull += culls > 0
        held = [set(h) for h in s["held"]]
        mono += any(u < 0 for row in s["uright"] for u in row); stereo += any(u >= 0 for row in s["uright"] for u in row)
        unheld += any(p not in held[k] for p, obs in enumerate(s["pt_obs"]) for k, _ in obs)
        unobserved += any(p is not None and k not in [o[0] for o in s["pt_obs"][p]] for k, h in enumerate(s["held"]) for p in h)
    assert 2 * with_cull >= len(scenes), with_cull                            # the chain is exercised
    assert mono == stereo == len(scenes) and unheld > 10 and unobserved > 10 and gone > 20 and not_erase > 0


@pytest.mark.parametrize("pin", cs.PINS, ids=lambda p: p.__name__)
def test_hand_built_scenes_give_the_rows_written_beside_them(pin):
    s, want = pin()
    for c, rows in zip(s["items"], want):
        got, order = cm.cull_keyframes(s, c)
        lit, lorder, lstate = cm.cull_keyframes_literal(s, c)
        assert got == rows and lit == rows and order == lorder and cm.replay(s, order) == lstate


@pytest.mark.parametrize("pin", cs.PINS[:11], ids=lambda p: p.__name__)
def test_scenes_1_to_11_fail_an_entry_state_or_consistent_table_implementation(pin):
    s, want = pin()
    wrong = [w for w in ("entry", "consistent") if [cm.cull_keyframes(s, c, w)[0] for c in s["items"]] != want]
    assert wrong and (pin is not cs.pin_inconsistent_tables or "consistent" in wrong)


def test_the_verdict_forms_are_equal_up_to_the_slot_limit():
    for n_mps in range(0, 8193):
        for n_red in {max(0, (9 * n_mps) // 10 - 1), (9 * n_mps) // 10, min(n_mps, (9 * n_mps) // 10 + 1), n_mps}:
            assert (float(n_red) > 0.9 * float(n_mps)) == (10 * n_red > 9 * n_mps), (n_mps, n_red)


def test_ratio_forms_differ_on_one_of_three():
    args = dict(found=1, visible=3, first_kf_id=5, nobs=9, live=True, cur_kf_id=6, th_obs=3)
    assert cm.cull_recent(ratio_form=cm.RATIO_FLOAT, **args) == cm.RECENT_KEEP     # 0.333f
    assert cm.cull_recent(ratio_form=cm.RATIO_INT, **args) == cm.RECENT_CULL_RATIO  # (float)(1 / 3) == 0
    # visible == 0: inf and NaN compare false in the float form; the integer form divides by zero unless the element is bad
    for found in (0, 4):
        assert cm.cull_recent(found, 0, 5, 9, True, 6, 3, cm.RATIO_FLOAT) == cm.RECENT_KEEP
        assert cm.cull_recent(found, 0, 5, 9, True, 6, 3, cm.RATIO_INT) == cm.RECENT_INVALID
        assert cm.cull_recent(found, 0, 5, 9, False, 6, 3, cm.RATIO_INT) == cm.RECENT_ERASE_BAD


def test_recent_branches_in_the_reference_s_order():
    f = lambda **kw: cm.cull_recent(**dict(dict(found=3, visible=4, first_kf_id=10, nobs=4, live=True, cur_kf_id=10, th_obs=3, ratio_form=0), **kw))
    assert f() == cm.RECENT_KEEP and f(live=False, found=0) == cm.RECENT_ERASE_BAD
    assert f(found=0, cur_kf_id=13, nobs=1) == cm.RECENT_CULL_RATIO            # the ratio comes before the age tests
    assert f(cur_kf_id=12, nobs=3) == cm.RECENT_CULL_OBS and f(cur_kf_id=12, nobs=4) == cm.RECENT_KEEP
    assert f(cur_kf_id=13, nobs=3) == cm.RECENT_CULL_OBS and f(cur_kf_id=13, nobs=4) == cm.RECENT_RETIRE
    assert f(cur_kf_id=11, nobs=0) == cm.RECENT_KEEP
    assert f(cur_kf_id=12, nobs=3, th_obs=2) == cm.RECENT_KEEP and f(cur_kf_id=12, nobs=2, th_obs=2) == cm.RECENT_CULL_OBS   # planes
    assert np.float32(1) / np.float32(4) == np.float32(0.25) and f(found=1) == cm.RECENT_KEEP   # 0.25f < 0.25f is false

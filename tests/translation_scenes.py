"""Synthetic TranslationOptimization inputs (fixed seeds): tests/pose_scenes.scene's frames (true pose, points, lines, planes, translation
perturbed) with a Manhattan rotation Rcw = the true rotation perturbed by at most max_rot_deg degrees, as DetectManhattan would supply it."""
import numpy as np

from tests import pose_scenes as ps
from tests import translation_model as tm


def scene(seed, max_rot_deg=0.5, margin=1e-4, c=None, **kw):
    """One frame.  Returns (fr, rcw (9,) f32, Rtrue, ttrue); kw goes to pose_scenes.scene.  When margin is set, asserts that every
    comparison of the model's last classification lies more than margin (relative) away from its threshold."""
    c = c or ps.params(nlevels=kw.get("nlevels", ps.NLEVELS), scale=kw.get("scale", ps.SCALE))
    fr, R, t = ps.scene(seed, margin=None, c=c, **kw)
    rng = np.random.default_rng(seed + 7919)
    rcw = (ps.rot(rng.normal(size=3), rng.uniform(0, max_rot_deg)) @ R).astype(np.float32).reshape(9)
    if margin is not None:
        check_margin(fr, c, rcw, margin)
    return fr, rcw, R, t


def check_margin(fr, c, rcw, margin=1e-4):
    rows = []
    tm.translation_optimization(fr, c, rcw, rows)
    for kind, idx, x2, th in rows:
        assert abs(x2 - th) > margin * th, ("chi2 too close to its threshold", kind, idx, x2, th)

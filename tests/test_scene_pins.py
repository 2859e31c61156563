"""The scene helpers' default outputs are pinned byte for byte: every existing parity test builds its inputs through them, so a change to a
helper (new parameters such as nlevels or the scale factor) must leave the arrays those tests have always used untouched."""
import hashlib

import numpy as np

from tests import line_match_scenes as lms
from tests import local_match_scenes as ls
from tests import match_scenes as ms
from tests import pose_scenes as ps
from tests import translation_scenes as ts


def digest(obj):
    """sha256 over every array / number reachable from obj (dicts in key order, sequences in order), dtype and shape included."""
    h = hashlib.sha256()

    def walk(o):
        if isinstance(o, dict):
            for k in sorted(o):
                h.update(repr(k).encode())
                walk(o[k])
        elif isinstance(o, (list, tuple)):
            h.update(b"[%d" % len(o))
            for v in o:
                walk(v)
        else:
            a = np.ascontiguousarray(np.asarray(o))
            h.update(str(a.dtype.descr if a.dtype.fields else a.dtype.str).encode() + repr(a.shape).encode())
            h.update(a.tobytes())

    walk(obj)
    return h.hexdigest()[:24]


def _outputs():
    from manhattanslam_amd import MATCH_PARAMS_DTYPE
    p = ms.params(None, 15, True, dtype=MATCH_PARAMS_DTYPE)
    lp = ls.params()
    lmp = lms.params()
    return {
        "match_params": p,
        "match_pair_11": ms.random_pair(11, p, n_cur=900, n_last=850),
        "match_pair_14": ms.random_pair(14, p, n_cur=1000, n_last=950, tz=0.3, cluster=True),
        "match_pair_18": ms.random_pair(18, p, n_cur=800, n_last=800, tz=-0.3, cluster=True),
        "local_params": lp,
        "local_frame_1": ls.random_frame(1, lp),
        "local_frame_7": ls.random_frame(7, lp, n_cur=500, n_local=3000, cluster=True),
        "local_frame_9": ls.random_frame(9, lp, n_cur=600, n_local=2000, conflict=True),
        "line_params": lmp,
        "line_pair_3": lms.frame_pair(3, lmp),
        "line_pair_5": lms.frame_pair(5, lmp, vertical=6, fwd=0.4),
        "line_local_4": lms.local_frame(4, lmp, n_kl=40, n_local=600),
        "line_local_6": lms.local_frame(6, lmp, n_kl=30, n_local=400, few=3),
        "pose_params": ps.params(),
        "pose_scene_1": ps.scene(1, margin=None),
        "pose_scene_5": ps.scene(5, n_pts=900, n_lines=20, n_planes=5, outliers=0.1, margin=None),
        "translation_scene_2": ts.scene(2, margin=None),
    }


# taken from the helpers before they gained their nlevels / scale / xcap parameters
PINNED = {
    "match_params": "b7d30d2b241d50b38c7dd2e2",
    "match_pair_11": "4bf880f7080ae71e544d7361",
    "match_pair_14": "351e36d8648c04db5ffeeb66",
    "match_pair_18": "6dd502d37a17b6d2a14511db",
    "local_params": "241cd92a2855b9988155d007",
    "local_frame_1": "94157e0d0cb7cceb45544208",
    "local_frame_7": "11b108e5316272bcddd395b4",
    "local_frame_9": "276e63139909c9a6fa82e7cb",
    "line_params": "c4ad999a56a4e96c00846bde",
    "line_pair_3": "cc08da149515a18dd7fa7391",
    "line_pair_5": "9ab8bf730fbfd0d8a7cef152",
    "line_local_4": "42b07e07579a5826f04926e1",
    "line_local_6": "d17d796a85e36415e979acb2",
    "pose_params": "a11b0ac58f8139a5abf43c9f",
    "pose_scene_1": "bf4219d255b40b8f7b5dab5e",
    "pose_scene_5": "b7bbcdf0c13af30312378bea",
    "translation_scene_2": "a61325e2c9e2915b14b34fbf",
}


def test_scene_helpers_default_outputs_are_pinned():
    got = {k: digest(v) for k, v in _outputs().items()}
    assert got == PINNED, {k: (got[k], PINNED.get(k)) for k in got if got[k] != PINNED.get(k)}

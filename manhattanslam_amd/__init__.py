"""MI355X-native RGB-D front end for ManhattanSLAM: ORB extractor + surfel fusion.

The product is the C-ABI shared library ``libmsl.so`` (hand-written HIP for gfx950, see
``include/msl.h``); this package is the thin Python host mirror of the reference's two
entry classes, used by the tests and ``bench.py``.  There is no CPU fallback: importing the
compute classes without the built library, or constructing them without an MI355X, raises.
"""
from ._lib import lib, MslError, KEYPOINT_DTYPE, SURFEL_DTYPE, SEED_DTYPE, device_count  # noqa: F401
from .orb import ORBextractor, frame_params  # noqa: F401
from .surfel import SurfelFusion, SurfelMap  # noqa: F401
from . import peac  # noqa: F401
from ._lib import PEAC_STATS_DTYPE  # noqa: F401
from . import match  # noqa: F401
from ._lib import MATCH_PARAMS_DTYPE, LOCAL_MATCH_PARAMS_DTYPE, LOCAL_TRACK_DTYPE  # noqa: F401
from ._lib import LINE_MATCH_PARAMS_DTYPE, KEYLINE_DTYPE, LINE_TRACK_DTYPE  # noqa: F401
from . import pose  # noqa: F401
from ._lib import POSE_PARAMS_DTYPE  # noqa: F401
from . import plane  # noqa: F401
from ._lib import PLANE_PARAMS_DTYPE  # noqa: F401
from . import plane_cloud  # noqa: F401
from ._lib import PLANE_CLOUD_PARAMS_DTYPE  # noqa: F401
from . import bow  # noqa: F401
from ._lib import BOW_MATCH_PARAMS_DTYPE  # noqa: F401
from . import reloc  # noqa: F401
from ._lib import KEYFRAME_MATCH_PARAMS_DTYPE  # noqa: F401
from . import pnp  # noqa: F401
from ._lib import PNP_PARAMS_DTYPE  # noqa: F401
from . import line3d  # noqa: F401
from ._lib import LINE3D_PARAMS_DTYPE  # noqa: F401
from . import triangulate  # noqa: F401
from ._lib import TRIANGULATE_PARAMS_DTYPE  # noqa: F401
from . import fuse  # noqa: F401
from ._lib import FUSE_PARAMS_DTYPE  # noqa: F401
from . import mappoint  # noqa: F401
from ._lib import REFRESH_PARAMS_DTYPE  # noqa: F401
from . import linefuse  # noqa: F401
from ._lib import LINE_FUSE_PARAMS_DTYPE  # noqa: F401
from . import localmap  # noqa: F401
from . import cull  # noqa: F401
from . import observations  # noqa: F401
from . import connections  # noqa: F401
from . import keyframe  # noqa: F401
from . import kfplanes  # noqa: F401

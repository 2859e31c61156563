"""Constants, tables and record layouts pinned against the reference's OWN source text (read as data: numbers and field names only).

The reference has no tests or golden vectors, but the numbers it hard-codes are part of its behaviour: the learned rBRIEF pattern, the patch and
border constants, the surfel-fusion macros, the field order of the records that cross the drop-in boundary, the matcher thresholds and the PEAC
defaults.  They were read out of the reference once into tests/golden/reference_pins.json (tests/golden/make_reference_pins.py regenerates it
from a reference tree), so these tests need no copy of the reference."""
import hashlib
import json
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pins():
    with open(os.path.join(ROOT, "tests", "golden", "reference_pins.json")) as f:
        return json.load(f)


def _const(text, name):
    m = re.search(r"\b" + re.escape(name) + r"\s*=\s*([-+0-9.eE]+)", text) or re.search(r"#define\s+" + re.escape(name) + r"\s+([-+0-9.eE]+)", text)
    assert m, name
    return float(m.group(1))


def test_rbrief_pattern_is_the_references_table(pins):
    ref = pins["rbrief_pattern"]
    ours = np.array([int(v) for v in re.findall(r"-?\d+", re.sub(r"//.*", "", open(os.path.join(ROOT, "include", "msl_orb_pattern.inc")).read()))], np.int32)
    assert ref["count"] == 1024 and hashlib.sha256(ours[-1024:].tobytes()).hexdigest() == ref["sha256_int32"]


def test_orb_constants(pins):
    o = pins["orb"]
    assert (o["PATCH_SIZE"], o["HALF_PATCH_SIZE"], o["EDGE_THRESHOLD"]) == (31, 15, 19)
    assert o["W"] == 30                                            # FAST cell size, src/ORBextractor.cc:726
    csrc = os.path.join(ROOT, "manhattanslam_amd", "csrc")
    hip = "".join(open(os.path.join(csrc, f)).read() for f in ("msl_orb_dev.h", "msl_orb.hip", "msl_orb_host.hip"))
    assert "const float Wc = 30;" in hip and "(int)(31 * h->scale[l])" in hip
    hdr = open(os.path.join(ROOT, "include", "msl.h")).read()
    assert int(o["FRAME_GRID_ROWS"]) == int(_const(hdr, "MSL_FRAME_GRID_ROWS")) == 48
    assert int(o["FRAME_GRID_COLS"]) == int(_const(hdr, "MSL_FRAME_GRID_COLS")) == 64


def test_surfel_fusion_macros(pins):
    assert pins["surfel_fusion"] == {"ITERATION_NUM": 3, "THREAD_NUM": 10, "SP_SIZE": 8, "MAX_ANGLE_COS": 0.1, "HUBER_RANGE": 0.4, "BASELINE": 0.5,
                                     "DISPARITY_ERROR": 4.0, "MIN_TOLERATE_DIFF": 0.1}
    csrc = os.path.join(ROOT, "manhattanslam_amd", "csrc")
    hip = "".join(open(os.path.join(csrc, f)).read() for f in ("msl_sf.h", "msl_sf_map_dev.h", "msl_sf_sp_dev.h", "msl_sf_superpixel.hip", "msl_sf_sp_assign.hip", "msl_sf_sp_seeds.hip",
                                                                    "msl_sf_sp_plane.hip", "msl_sf_fuse.hip", "msl_sf_compact.hip", "msl_sf_replay.hip", "msl_sf_map.hip", "msl_sf_handle.h",
                                                                    "msl_sf_plan.h", "msl_surfel.hip", "msl_sf_store.hip", "msl_sf_hostvec.hip", "msl_sf_debug.hip"))
    assert "constexpr int SP = 8;" in hip and "constexpr int NCHUNK = 10;" in hip
    assert "MAX_ANGLE_COS = 0.1, HUBER_RANGE = 0.4, MIN_TOLERATE_DIFF = 0.1" in hip
    assert "halfF = 0.5f * cameraF" in hip and "/ halfF * 4.0f" in hip          # BASELINE and DISPARITY_ERROR as exact float factors in k_fuse
    assert hip.count("for (int it = 0; it < 3; it++)") >= 1                      # ITERATION_NUM passes of (pixels, seeds)
    assert pins["surfel_mapping_drift_free_poses"] == 10                          # src/SurfelMapping.cpp: driftFreePoses(10)
    assert "driftFreePoses(10)" in open(os.path.join(ROOT, "manhattanslam_amd", "adapter", "SurfelMapping.cpp")).read()


def test_record_layouts_follow_the_references_structs(pins):
    from manhattanslam_amd._lib import SEED_DTYPE, SURFEL_DTYPE
    ref = pins["surfel_fields"]
    assert [n for _, n in ref] == list(SURFEL_DTYPE.names)
    assert [("f" if t == "float" else "i") for t, _ in ref] == [SURFEL_DTYPE[n].kind for n in SURFEL_DTYPE.names]
    ref = pins["superpixel_seed_fields"]
    ours = [n for n in SEED_DTYPE.names if n != "_pad"]
    assert [n for _, n in ref] == ours
    assert [{"float": "f", "int": "i", "bool": "u"}[t] for t, _ in ref] == [SEED_DTYPE[n].kind for n in ours]
    assert SURFEL_DTYPE.itemsize == 56 and SEED_DTYPE.itemsize == 64


def test_matcher_constants(pins):
    m = pins["matcher"]
    assert (m["TH_HIGH"], m["TH_LOW"], m["HISTO_LENGTH"]) == (100, 50, 30)
    assert "constexpr int TH_HIGH = 100, HISTO_LENGTH = 30;" in open(os.path.join(ROOT, "manhattanslam_amd", "csrc", "msl_match.hip")).read()


def test_peac_defaults_are_the_references(pins):
    from manhattanslam_amd import peac
    p = peac.default_params()[0]
    ps = pins["peac_param_set"]
    assert p["depth_sigma"] == ps["depthSigma"] and p["std_tol_init"] == ps["stdTol_init"] and p["std_tol_merge"] == ps["stdTol_merge"]
    assert p["z_near"] == ps["z_near"] and p["z_far"] == ps["z_far"] and p["depth_alpha"] == ps["depthAlpha"] and p["depth_change_tol"] == ps["depthChangeTol"]
    assert p["angle_near"] == math.radians(ps["angle_near_deg"]) and p["angle_far"] == math.radians(ps["angle_far_deg"])
    assert p["similarity_th_merge"] == math.cos(math.radians(ps["similarityTh_merge_deg"])) and p["similarity_th_refine"] == math.cos(math.radians(ps["similarityTh_refine_deg"]))
    assert p["init_loose"] == 0 and ps["init_strict"]
    pf = pins["peac_plane_fitter"]
    assert (p["max_step"], p["min_support"], p["window_w"], p["window_h"]) == (pf["maxStep"], pf["minSupport"], pf["windowWidth"], pf["windowHeight"])
    assert p["do_refine"] == 1 and pf["doRefine"] and p["erode_type"] == 2      # ERODE_ALL_BORDER is the third enumerator
    assert pf["ERODE_ALL_BORDER"] == p["erode_type"]

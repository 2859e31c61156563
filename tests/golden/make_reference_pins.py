#!/usr/bin/env python3
"""Regenerates tests/golden/reference_pins.json: the constants, tables and record layouts the reference hard-codes, read from its source text as
data (numbers and field names only; the 1024-entry rBRIEF table as its count and SHA-256).  tests/test_reference_pins.py checks the project
against this file, so the suite needs no copy of the reference.

    python tests/golden/make_reference_pins.py /path/to/ManhattanSLAM
"""
import hashlib
import json
import os
import re
import sys

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_pins.json")


def _const(text, name):
    m = re.search(r"\b" + re.escape(name) + r"\s*=\s*([-+0-9.eE]+)", text) or re.search(r"#define\s+" + re.escape(name) + r"\s+([-+0-9.eE]+)", text)
    assert m, name
    return float(m.group(1))


def _fields(struct_text):
    out = []
    for decl in re.findall(r"\b(float|int|bool)\s+([^;]+);", struct_text):
        for name in decl[1].split(","):
            out.append([decl[0], name.split("=")[0].strip()])
    return out


def pins(ref_dir):
    ref = lambda path: open(os.path.join(ref_dir, path), errors="replace").read()
    out = {}

    src = ref("src/ORBextractor.cc")
    body = src[src.index("bit_pattern_31_[256 * 4]"):]
    body = body[body.index("{") + 1:body.index("};")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    pat = np.array([int(v) for v in re.findall(r"-?\d+", body)], np.int32)
    out["rbrief_pattern"] = {"count": int(pat.size), "sha256_int32": hashlib.sha256(pat.tobytes()).hexdigest()}
    fr = ref("include/Frame.h")
    out["orb"] = {"PATCH_SIZE": _const(src, "PATCH_SIZE"), "HALF_PATCH_SIZE": _const(src, "HALF_PATCH_SIZE"), "EDGE_THRESHOLD": _const(src, "EDGE_THRESHOLD"),
                  "W": _const(src, "const float W"), "FRAME_GRID_ROWS": _const(fr, "FRAME_GRID_ROWS"), "FRAME_GRID_COLS": _const(fr, "FRAME_GRID_COLS")}

    h = ref("include/SurfelFusion.h")
    out["surfel_fusion"] = {k: _const(h, k) for k in ("ITERATION_NUM", "THREAD_NUM", "SP_SIZE", "MAX_ANGLE_COS", "HUBER_RANGE", "BASELINE",
                                                      "DISPARITY_ERROR", "MIN_TOLERATE_DIFF")}
    out["surfel_mapping_drift_free_poses"] = int(re.search(r"driftFreePoses\((\d+)\)", ref("src/SurfelMapping.cpp")).group(1))

    s = ref("include/Surfel.h")
    out["surfel_fields"] = _fields(s[s.index("struct Surfel"):s.index("};")])
    body = h[h.index("struct SuperpixelSeed"):]
    out["superpixel_seed_fields"] = _fields(body[:body.index("};")])

    src = ref("src/ORBmatcher.cc")
    out["matcher"] = {k: _const(src, "ORBmatcher::" + k) for k in ("TH_HIGH", "TH_LOW", "HISTO_LENGTH")}

    ps = ref("include/peac/AHCParamSet.hpp")
    ctor = ps[ps.index("ParamSet() :"):ps.index("initType(INIT_STRICT)")]
    num = lambda text, name: float(re.search(name + r"\(([-+0-9.eE]+)\)", text).group(1))
    deg = lambda name: float(re.search(name + r"\((?:std::cos\()?MACRO_DEG2RAD\(([0-9.]+)\)", ctor).group(1))
    out["peac_param_set"] = {**{k: num(ctor, k) for k in ("depthSigma", "stdTol_init", "stdTol_merge", "z_near", "z_far", "depthAlpha", "depthChangeTol")},
                             **{k + "_deg": deg(k) for k in ("angle_near", "angle_far", "similarityTh_merge", "similarityTh_refine")},
                             "init_strict": "INIT_STRICT" in ps}
    pf = ref("include/peac/AHCPlaneFitter.hpp")
    ctor = pf[pf.index("maxStep(100000)") - 200:pf.index("erodeType(ERODE_ALL_BORDER)") + 40]
    out["peac_plane_fitter"] = {**{k: num(ctor, k) for k in ("maxStep", "minSupport", "windowWidth", "windowHeight")},
                                "doRefine": "doRefine(true)" in ctor,
                                "ERODE_ALL_BORDER": int(re.search(r"ERODE_ALL_BORDER\s*=\s*(\d+)", pf).group(1))}
    return out


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    with open(OUT, "w") as f:
        json.dump(pins(sys.argv[1]), f, indent=1)
        f.write("\n")

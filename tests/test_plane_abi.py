"""msl_plane_associate[_batch] and msl_manhattan_detect[_batch] are part of the C ABI: exported by libmsl.so, declared in include/msl.h and
bound in _lib.  They refuse an invalid call before they touch a device, through the device-indexed forms on host memory: every limit and every NULL of a required array is refused with the argument named, an unsorted host-memory table with the table
and its frame named, and the outputs and the in/out arrays keep their bytes.  The optional arrays and a table count beyond its capacity are
not invalid.  The limits of the plane chain stand once in Python (plane) and once in C++ (csrc/msl_plane_tables.h) and equal msl.h's
Limits: paragraphs.  No launch is asserted (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import abi_refusals
from tests import kfplanes_scenes as ks
from tests.abi_refusals import put

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PA, MD = "msl_plane_associate", "msl_manhattan_detect"
SH = dict(n_frames=2, pcap=8, mcap=8, fcap=4, qcap=4, kcap=2, ptcap=16)
OUT = {PA: ("nmatches", "plane_w", "plane_has", "pM_out"), MD: ("found", "full", "choice")}
INOUT = {PA: ("plane_match",), MD: ("Rcw",)}
OPTIONAL = {PA: "pM_out", MD: "choice"}
INT_MAX = 2 ** 31 - 1
NAMES = ("msl_plane_associate", "msl_plane_associate_batch", "msl_manhattan_detect", "msl_manhattan_detect_batch")


def test_exported_declared_and_bound():
    from manhattanslam_amd import _header, _lib
    decl = _header.declarations(_header.text("msl.h"))
    dll = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert decl[n][0] == "int", n
        assert hasattr(dll, n), n
        assert n in _lib.SIGNATURES, n


def test_argument_counts_match_the_header():
    from manhattanslam_amd import _header, _lib
    decl = _header.declarations(_header.text("msl.h"))
    for n in NAMES:
        assert len(decl[n][1]) == len(_lib.SIGNATURES[n][1]), n


def test_params_record_is_five_floats():
    from manhattanslam_amd import PLANE_PARAMS_DTYPE
    assert PLANE_PARAMS_DTYPE.itemsize == 20 and PLANE_PARAMS_DTYPE.names == ("d_th", "a_th", "ver_th", "par_th", "mf_ver_th")


@pytest.fixture(scope="module")
def scene():
    """Two small frames that a device would accept as they stand: counts inside their capacities, offsets ascending, both tables sorted over
    all of their fcap / qcap entries (so that a count beyond the capacity still names sorted entries)."""
    from manhattanslam_amd import plane
    rng = np.random.default_rng(7)
    F, P, M, FC, QC, K, PT = (SH[k] for k in ("n_frames", "pcap", "mcap", "fcap", "qcap", "kcap", "ptcap"))
    unit = lambda shape: (lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True))(rng.normal(size=shape + (3,)))
    coef = lambda shape: np.concatenate([unit(shape), rng.uniform(-2, 2, shape + (1,))], -1).astype(np.float32)
    n_map = np.array([4, 6], np.int32)
    off = np.zeros((F, M + 1), np.int32)
    for f in range(F):
        off[f] = np.minimum(2 * np.arange(M + 1), 2 * n_map[f])
    match = np.full((F, P, 3), -1, np.int32)
    match[:, :3, 0] = np.arange(3)
    full = np.zeros((F, FC, plane.FULL_STRIDE), np.int32)
    full[:, :, :3] = [(0, 1, 2), (0, 1, 3), (1, 2, 3), (1, 2, 4)][:FC]
    full[:, :, 3] = [0, 1, 0, 1][:FC]
    full[:, :, 4:] = [0, 1, 2]
    part = np.zeros((F, QC, plane.PART_STRIDE), np.int32)
    part[:, :, :2] = [(0, 1), (0, 2), (1, 3), (2, 3)][:QC]
    part[:, :, 2] = [1, 0, 1, 0][:QC]
    part[:, :, 3:] = [0, 1]
    a = dict(params=plane.plane_params(0.2, 0.9, 0.08, 0.9, 0.1), plane_coef=coef((F, P)), plane_npts=rng.integers(10, 100, (F, P)).astype(np.int32),
             n_planes=np.array([3, 5], np.int32), Tcw=np.tile(np.eye(4, dtype=np.float32)[:3].reshape(12), (F, 1)), mp_w=coef((F, M)),
             mp_flags=np.ones((F, M), np.uint8), mp_pt_off=off, mp_pts=rng.uniform(-3, 3, (F, PT, 3)).astype(np.float32), n_map=n_map,
             plane_match=match, full_tab=full, n_full=np.array([1, 3], np.int32), part_tab=part, n_part=np.array([2, 3], np.int32),
             kf_Rwc=np.tile(np.eye(3, dtype=np.float32).reshape(9), (F, K, 1)), kf_coef=coef((F, K, P)),
             kf_npts=rng.integers(10, 100, (F, K, P)).astype(np.int32), Rcw=ks.host_filled((F, 9), np.float32))
    return a


def outputs(entry):
    F, P = SH["n_frames"], SH["pcap"]
    shapes = dict(nmatches=((F,), np.int32), plane_w=((F, P, 12), np.float32), plane_has=((F, P), np.uint8), pM_out=((F, P, 4), np.float32),
                  found=((F,), np.int32), full=((F,), np.int32), choice=((F, 6), np.int32))
    return {k: ks.host_filled(*shapes[k]) for k in OUT[entry]}


def run(entry, scene, **over):
    """abi_refusals.call on the scene: (return code, msl_last_error())."""
    return abi_refusals.call(entry, SH, scene, outputs(entry), inout=INOUT[entry], **over)


def refused(entry, scene, **over):
    return abi_refusals.refused(entry, SH, scene, outputs(entry), inout=INOUT[entry], **over)


LIMITS = {PA: dict(n_frames=INT_MAX, pcap=64, mcap=4096, ptcap=1 << 22), MD: dict(n_frames=INT_MAX, pcap=64, mcap=4096, fcap=65536, qcap=65536, kcap=4096)}


@pytest.mark.parametrize("entry", [PA, MD])
def test_every_limit_is_refused_with_the_argument_named(scene, entry):
    from manhattanslam_amd import _header
    assert set(LIMITS[entry]) == {n for t, n in _header.declarations(_header.text("msl.h"))[entry][1][1:] if t == "int"}
    for name, limit in LIMITS[entry].items():
        for value in (0,) if name == "n_frames" else (0, limit + 1):
            assert refused(entry, scene, **{name: value}) == f"{entry}: {name} {value} outside 1 .. {limit}"


@pytest.mark.parametrize("entry", [PA, MD])
def test_every_null_of_a_required_array_is_refused_with_its_name(scene, entry):
    from manhattanslam_amd import _header
    pointers = [n for t, n in _header.declarations(_header.text("msl.h"))[entry][1][1:] if t.endswith("*")]
    assert len(pointers) == {PA: 14, MD: 18}[entry] and OPTIONAL[entry] in pointers
    for n in pointers:
        if n != OPTIONAL[entry]:
            assert refused(entry, scene, **{n: None}) == f"{entry}: {n} is NULL"


def test_an_unsorted_host_table_is_refused_with_the_table_and_the_frame_named(scene):
    swap = lambda i, j: lambda x: x.__setitem__((1, [i, j]), x[1, [j, i]])
    assert refused(MD, scene, full_tab=put((1, 1, slice(0, 3)), [3, 1, 0])) == f"{MD}: full_tab[1] is not sorted by its keys at entry 1"
    assert refused(MD, scene, full_tab=swap(1, 2)) == f"{MD}: full_tab[1] is not sorted by its keys at entry 2"
    assert refused(MD, scene, part_tab=put((1, 1, slice(0, 2)), [2, 0])) == f"{MD}: part_tab[1] is not sorted by its keys at entry 1"
    assert refused(MD, scene, part_tab=swap(1, 2)) == f"{MD}: part_tab[1] is not sorted by its keys at entry 2"


def test_optional_arrays_and_counts_beyond_the_capacity_are_not_invalid(scene):
    """What the check lets through goes on to the device: without one the call fails with another code than MSL_ERR_INVALID."""
    assert run(PA, scene, pM_out=None)[0] != -1
    assert run(MD, scene, choice=None)[0] != -1
    assert run(MD, scene, n_full=put(1, SH["fcap"] + 3))[0] != -1              # clamped, and the fcap entries are sorted
    assert run(MD, scene, n_part=put(0, -2), n_full=put(0, -1))[0] != -1       # clamped to 0: no entry is checked
    # beyond the clamped count a table is not checked
    assert run(MD, scene, full_tab=put((0, 2, slice(0, 3)), [9, 1, 0]))[0] != -1


def test_the_handle_forms_refuse_a_null_handle():
    from manhattanslam_amd import _lib
    for entry in (PA, MD):
        args = [0 if t in (C.c_int, C.c_uint) else None for t in _lib.SIGNATURES[entry][1][1:]]
        assert getattr(_lib.lib, entry)(None, *args) == -1
        assert _lib.lib.msl_last_error().decode() == f"{entry}: h is NULL"


def test_the_chain_s_limits_stand_once_and_are_the_header_s():
    from manhattanslam_amd import keyframe, kfplanes, plane
    for n in ("MAX_FRAMES", "MAX_PCAP", "MAX_MCAP", "MAX_FCAP", "MAX_QCAP", "MAX_KCAP"):
        assert getattr(kfplanes, n) is getattr(plane, n), n
    assert keyframe.MAX_PCAP is plane.MAX_PCAP
    p = plane
    text = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", "msl.h")).read())
    groups = lambda pattern: tuple(int(x) for x in re.search(pattern, text).groups())
    assert groups(r"Limits: pcap <= (\d+), mcap <= (\d+), ptcap <= 2\^(\d+); larger values") == (p.MAX_PCAP, p.MAX_MCAP, p.MAX_PTCAP.bit_length() - 1)
    assert groups(r"Limits: pcap <= (\d+), mcap <= (\d+), fcap <= (\d+), qcap <= (\d+), kcap <= (\d+); larger values") == (
        p.MAX_PCAP, p.MAX_MCAP, p.MAX_FCAP, p.MAX_QCAP, p.MAX_KCAP)
    assert groups(r"Limits: n_frames <= (\d+), n_vertices <= MSL_PLANE_CLOUD_MAX_VERTICES, max_planes <= (\d+), pcap <= (\d+), mcap <= (\d+), "
                  r"ptcap and fptcap <= 2\^(\d+),") == (p.MAX_FRAMES, p.MAX_PCAP, p.MAX_PCAP, p.MAX_MCAP, p.MAX_PTCAP.bit_length() - 1)
    assert groups(r"Limits: n_frames in 1 \.\. (\d+), pcap <= (\d+), mcap <= (\d+), kcap <= (\d+) \(each at least 1\), mode one of MSL_KFPLANES_\*") == (
        p.MAX_FRAMES, p.MAX_PCAP, p.MAX_MCAP, p.MAX_KCAP)
    assert groups(r"Limits: n_frames in 1 \.\. (\d+), pcap <= (\d+), mcap <= (\d+), fcap <= (\d+), qcap <= (\d+), kcap <= (\d+) \(each at least 1\); refusals") == (
        p.MAX_FRAMES, p.MAX_PCAP, p.MAX_MCAP, p.MAX_FCAP, p.MAX_QCAP, p.MAX_KCAP)
    assert p.MAX_PTCAP == 1 << (p.MAX_PTCAP.bit_length() - 1)
    # the C++ side: one definition, the same numbers, and the same entry layout
    src = open(os.path.join(ROOT, "manhattanslam_amd", "csrc", "msl_plane_tables.h")).read()
    value = lambda n: eval(re.search(r"\b%s = ([0-9 <]+)[,;]" % n, src).group(1))
    assert [value(n) for n in ("MAX_PLANE_FRAMES", "MAX_PCAP", "MAX_PLANE_MCAP", "MAX_PLANE_PTCAP", "MAX_FCAP", "MAX_QCAP", "MAX_PLANE_KCAP")] == [
        p.MAX_FRAMES, p.MAX_PCAP, p.MAX_MCAP, p.MAX_PTCAP, p.MAX_FCAP, p.MAX_QCAP, p.MAX_KCAP]
    assert (value("FULL"), value("PART")) == (p.FULL_W, p.PART_W) and "return 2 * w + 1;" in src
    assert (p.FULL_STRIDE, p.PART_STRIDE) == (2 * p.FULL_W + 1, 2 * p.PART_W + 1)

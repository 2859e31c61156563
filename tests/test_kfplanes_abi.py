"""msl_keyframe_planes and msl_manhattan_observe are part of the C ABI: exported by libmsl.so, declared in include/msl.h and bound in _lib; the
two forms differ in their first argument only; the record has the header's layout, the constants its values, the Python wrapper its names,
and the arrays the types of the entries they chain with.  Their refusals, through the device-indexed forms on host memory, which check before
they touch a device: every limit, every NULL and every index defect of a host-memory call is refused with the field named, and the outputs
and the in/out arrays keep their bytes.  No launch (no GPU needed)."""
import ctypes as C
import re

import numpy as np
import pytest

from tests import abi_refusals
from tests import kfplanes_model as kp
from tests import kfplanes_scenes as ks
from tests.abi_refusals import put

NAMES = {"msl_keyframe_planes": 30, "msl_manhattan_observe": 26}


def test_exported_declared_and_bound():
    from manhattanslam_amd import _header, _lib
    dll = C.CDLL(_lib.LIB_PATH)
    decl = _header.declarations(_header.text("msl.h"))
    for base, count in NAMES.items():
        for n in (base, base + "_batch"):
            assert decl[n][0] == "int" and hasattr(dll, n), n
            res, args = _lib.SIGNATURES[n]
            assert res is C.c_int and len(args) == len(decl[n][1]) == count, n
            assert getattr(_lib.lib, n).argtypes == args
        a, b = decl[base][1], decl[base + "_batch"][1]
        assert a[0] == ("msl_match *", "h") and b[0] == ("int", "device") and a[1:] == b[1:]


def test_record_layout_is_the_header_s():
    from manhattanslam_amd import _lib, kfplanes
    r = _lib.RECORDS["msl_kfplanes_frame"]
    assert r.names == ("enable", "kf_slot", "kf_id", "_pad") and r.itemsize == 16
    assert all(r.fields[n] == (np.dtype("<i4"), 4 * i) for i, n in enumerate(r.names)) and kfplanes.KFPLANES_FRAME_DTYPE is r
    rec = kfplanes.frame_records([dict(kf_slot=3, kf_id=9), dict(enable=0, kf_slot=1, kf_id=2)])
    assert rec.tolist() == [(1, 3, 9, 0), (0, 1, 2, 0)]


def test_argument_order_constants_and_types_are_the_wrapper_s():
    import manhattanslam_amd as m
    from manhattanslam_amd import _header, kfplanes
    assert m.kfplanes is kfplanes and all(callable(getattr(kfplanes, n)) for n in kfplanes.__all__ if n[0].islower())
    src = _header.text("msl.h")
    decl = _header.declarations(src)
    names = [x[1] for x in decl["msl_keyframe_planes"][1]]
    assert names[1:6] == ["n_frames", "pcap", "mcap", "kcap", "mode"] and tuple(names[6:12]) == kfplanes.PLANES_IN_KEYS and names[12] == "mem"
    assert tuple(names[13:21]) == kfplanes.PLANES_INOUT_KEYS and tuple(names[21:29]) == kfplanes.PLANES_OUT_KEYS and names[29] == "out_mem"
    assert tuple(kfplanes.planes_outputs(1, 1)) == kfplanes.PLANES_OUT_KEYS == tuple(kp.planes_outputs(1, 1))
    names = [x[1] for x in decl["msl_manhattan_observe"][1]]
    assert names[1:8] == ["n_frames", "pcap", "mcap", "fcap", "qcap", "kcap", "params"] and tuple(names[8:15]) == kfplanes.OBSERVE_IN_KEYS
    assert names[15] == "mem" and tuple(names[16:20]) == kfplanes.OBSERVE_INOUT_KEYS and tuple(names[20:25]) == kfplanes.OBSERVE_OUT_KEYS
    assert names[25] == "out_mem" and tuple(kfplanes.observe_outputs(1, 1)) == kfplanes.OBSERVE_OUT_KEYS == tuple(kp.observe_outputs(1, 1))
    define = lambda n: int(re.search(r"#define\s+%s\s+(\d+)\b" % n, src).group(1))
    for mod in (kfplanes, kp):
        assert [define("MSL_KFPLANES_" + n) for n in ("KEYFRAME", "INIT")] == [mod.KEYFRAME, mod.INIT]
        assert [define("MSL_KFPLANES_" + n) for n in ("SKIPPED", "HELD", "NEW", "NO_ROOM")] == [mod.SKIPPED, mod.HELD, mod.NEW, mod.NO_ROOM]
        assert [define("MSL_MANHATTAN_" + n) for n in ("FULL_NO_ROOM", "PART_NO_ROOM")] == [mod.FULL_NO_ROOM, mod.PART_NO_ROOM]
    # the arrays are, name for name and type for type (an in/out array drops the const), those of the entries they chain with
    bare = lambda t: t.replace("const ", "")
    planes = {n: t for t, n in decl["msl_keyframe_planes"][1]}
    observe = {n: t for t, n in decl["msl_manhattan_observe"][1]}
    assoc = {n: t for t, n in decl["msl_plane_associate"][1]}
    detect = {n: t for t, n in decl["msl_manhattan_detect"][1]}
    merge = {n: t for t, n in decl["msl_map_plane_merge"][1]}
    decide = {n: t for t, n in decl["msl_keyframe_decision"][1]}
    for k in ("plane_coef", "n_planes", "Tcw", "plane_match", "mp_w", "mp_flags", "n_map"):
        assert bare(planes[k]) == bare(assoc[k]) and (k not in observe or observe[k] == "const " + bare(assoc[k])), k
    for k in ("plane_coef", "plane_npts", "n_planes"):
        assert planes[k] == detect[k], k
    for k in ("kf_Rwc", "kf_coef", "kf_npts"):
        assert "const " + planes[k] == detect[k], k
    for k in ("full_tab", "n_full", "part_tab", "n_part"):
        assert "const " + observe[k] == detect[k], k
    assert planes["plane_outlier"] == "const " + decide["plane_outlier"] and planes["plane_match"] == decide["plane_match"]
    assert "const " + planes["merge_into"] == merge["merge_into"] and "const " + planes["Twc"] == merge["Twc"]
    assert observe["kf_plane_match"] == "const " + planes["kf_plane_match"] == detect["plane_match"]
    assert observe["mp_first_kf"] == "const " + planes["mp_first_kf"] and observe["params"] == detect["params"] and observe["frames"] == planes["frames"]


def test_limits_are_the_header_s():
    import os
    from manhattanslam_amd import kfplanes
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(root, "include", "msl.h")).read())
    line = re.search(r"Limits: n_frames in 1 \.\. (\d+), pcap <= (\d+), mcap <= (\d+), kcap <= (\d+) \(each at least 1\), mode one of MSL_KFPLANES_\*", text)
    assert tuple(int(x) for x in line.groups()) == (kfplanes.MAX_FRAMES, kfplanes.MAX_PCAP, kfplanes.MAX_MCAP, kfplanes.MAX_KCAP)
    line = re.search(r"Limits: n_frames in 1 \.\. (\d+), pcap <= (\d+), mcap <= (\d+), fcap <= (\d+), qcap <= (\d+), kcap <= (\d+) \(each at least 1\); refusals", text)
    assert tuple(int(x) for x in line.groups()) == (kfplanes.MAX_FRAMES, kfplanes.MAX_PCAP, kfplanes.MAX_MCAP, kfplanes.MAX_FCAP, kfplanes.MAX_QCAP,
                                                    kfplanes.MAX_KCAP)
    det = re.search(r"Limits: pcap <= (\d+), mcap <= (\d+), fcap <= (\d+), qcap <= (\d+), kcap <= (\d+); larger values", text)     # msl_manhattan_detect's
    assert tuple(int(x) for x in det.groups()) == (kfplanes.MAX_PCAP, kfplanes.MAX_MCAP, kfplanes.MAX_FCAP, kfplanes.MAX_QCAP, kfplanes.MAX_KCAP)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    from manhattanslam_amd import kfplanes, plane
    fr = ks.ragged()
    caps, a = kfplanes.pack([fr[4], fr[5]], ks.PCAP, ks.MCAP, ks.FCAP, ks.QCAP, ks.KCAP)
    a["kf_plane_match"] = a["plane_match"].copy()
    a["params"] = plane.plane_params(0.2, 0.9, 0.08, 0.9, ks.TH)
    sh = dict(n_frames=2, pcap=ks.PCAP, mcap=ks.MCAP, fcap=ks.FCAP, qcap=ks.QCAP, kcap=ks.KCAP, mode=kp.KEYFRAME)
    return a, sh


def refused(entry, scene, **over):
    from manhattanslam_amd import kfplanes
    arrays, sh = scene
    planes = entry == "msl_keyframe_planes"
    out = kfplanes.planes_outputs(2, ks.PCAP, ks.host_filled) if planes else kfplanes.observe_outputs(2, ks.PCAP, ks.host_filled)
    return abi_refusals.refused(entry, sh, arrays, out, inout=kfplanes.PLANES_INOUT_KEYS if planes else kfplanes.OBSERVE_INOUT_KEYS, **over)


LIMITS = {"msl_keyframe_planes": [("n_frames", 0, "n_frames 0 outside 1 .. 65535"), ("n_frames", 65536, "n_frames 65536 outside 1 .. 65535"),
                                  ("pcap", 0, "pcap 0 outside 1 .. 64"), ("pcap", 65, "pcap 65 outside 1 .. 64"),
                                  ("mcap", 0, "mcap 0 outside 1 .. 4096"), ("mcap", 4097, "mcap 4097 outside 1 .. 4096"),
                                  ("kcap", 0, "kcap 0 outside 1 .. 4096"), ("kcap", 4097, "kcap 4097 outside 1 .. 4096"),
                                  ("mode", 2, "mode 2 is not an MSL_KFPLANES_* mode"), ("mode", -1, "mode -1 is not an MSL_KFPLANES_* mode")],
          "msl_manhattan_observe": [("n_frames", 0, "n_frames 0 outside 1 .. 65535"), ("n_frames", 65536, "n_frames 65536 outside 1 .. 65535"),
                                    ("pcap", 0, "pcap 0 outside 1 .. 64"), ("pcap", 65, "pcap 65 outside 1 .. 64"),
                                    ("mcap", 0, "mcap 0 outside 1 .. 4096"), ("mcap", 4097, "mcap 4097 outside 1 .. 4096"),
                                    ("fcap", 0, "fcap 0 outside 1 .. 65536"), ("fcap", 65537, "fcap 65537 outside 1 .. 65536"),
                                    ("qcap", 0, "qcap 0 outside 1 .. 65536"), ("qcap", 65537, "qcap 65537 outside 1 .. 65536"),
                                    ("kcap", 0, "kcap 0 outside 1 .. 4096"), ("kcap", 4097, "kcap 4097 outside 1 .. 4096")]}


@pytest.mark.parametrize("entry", sorted(NAMES))
def test_every_limit_is_refused_with_the_field_named(scene, entry):
    from manhattanslam_amd import _header
    assert {l[0] for l in LIMITS[entry]} == {n for t, n in _header.declarations(_header.text("msl.h"))[entry][1][1:] if t == "int"}
    for field, value, msg in LIMITS[entry]:
        assert refused(entry, scene, **{field: value}) == f"{entry}: {msg}"


@pytest.mark.parametrize("entry", sorted(NAMES))
def test_every_null_is_refused_with_the_field_named(scene, entry):
    from manhattanslam_amd import _header
    pointers = [n for t, n in _header.declarations(_header.text("msl.h"))[entry][1][1:] if t.endswith("*")]
    assert len(pointers) == {"msl_keyframe_planes": 22, "msl_manhattan_observe": 17}[entry]
    for n in pointers:
        assert refused(entry, scene, **{n: None}) == f"{entry}: {n} is NULL"


def test_index_defects_of_a_host_memory_call_are_refused(scene):
    kq, mo = "msl_keyframe_planes", "msl_manhattan_observe"
    for e in (kq, mo):
        assert refused(e, scene, n_planes=put(1, ks.PCAP + 1)) == f"{e}: n_planes[1] is {ks.PCAP + 1} outside 0 .. pcap = {ks.PCAP}"
        assert refused(e, scene, n_planes=put(0, -1)) == f"{e}: n_planes[0] is -1 outside 0 .. pcap = {ks.PCAP}"
        assert refused(e, scene, n_map=put(0, ks.MCAP + 1)) == f"{e}: n_map[0] is {ks.MCAP + 1} outside 0 .. mcap = {ks.MCAP}"
        assert refused(e, scene, frames=put(1, (1, ks.KCAP, 3, 0))) == f"{e}: frames[1].kf_slot is keyframe {ks.KCAP} of {ks.KCAP}"
        assert refused(e, scene, frames=put(0, (1, -1, 3, 0))) == f"{e}: frames[0].kf_slot is keyframe -1 of {ks.KCAP}"
        assert refused(e, scene, frames=put(0, (1, 0, -3, 0))) == f"{e}: frames[0].kf_id is -3, below 0"
    assert refused(kq, scene, plane_match=put((0, 1, 2), 10)) == f"{kq}: plane_match[0][1][2] is row 10 of 10"
    assert refused(kq, scene, plane_match=put((1, 11, 0), -2)) == f"{kq}: plane_match[1][11][0] is row -2 of 30"
    assert refused(mo, scene, kf_plane_match=put((1, 3, 0), 30)) == f"{mo}: kf_plane_match[1][3][0] is row 30 of 30"
    assert refused(mo, scene, n_full=put(1, ks.FCAP + 1)) == f"{mo}: n_full[1] is {ks.FCAP + 1} outside 0 .. fcap = {ks.FCAP}"
    assert refused(mo, scene, n_part=put(0, -1)) == f"{mo}: n_part[0] is -1 outside 0 .. qcap = {ks.QCAP}"
    assert refused(mo, scene, full_tab=put((1, 4, 0), 29)) == f"{mo}: full_tab[1] is not sorted by its keys at entry 4"
    assert refused(mo, scene, full_tab=put((1, 0), [5, 4, 6, 0, 0, 0, 0])) == f"{mo}: full_tab[1] is not sorted by its keys at entry 0"
    assert refused(mo, scene, part_tab=put((1, 3), scene[0]["part_tab"][1, 2])) == f"{mo}: part_tab[1] is not sorted by its keys at entry 3"


def test_the_handle_forms_refuse_a_null_handle():
    from manhattanslam_amd import _lib
    for entry, count in NAMES.items():
        args = [0 if t in (C.c_int, C.c_uint) else None for t in _lib.SIGNATURES[entry][1][1:]]
        assert len(args) == count - 1 and getattr(_lib.lib, entry)(None, *args) == -1
        assert _lib.lib.msl_last_error().decode() == f"{entry}: h is NULL"

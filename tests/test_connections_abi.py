"""msl_connections_apply and msl_fuse_targets are part of the C ABI: exported by libmsl.so, declared in include/msl.h and bound in _lib; the
two forms of each differ in their first argument only; the arrays they share with msl_covisibility, msl_local_keyframes and
msl_fuse_candidates have their names and types, without const where they are written here.  Their refusals, through the device-indexed
forms on host memory, which check before they touch a device: every limit, every NULL and every index defect of a host-memory call is
refused with the field named, and the in-place arrays and the outputs keep their bytes.  No launch (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import abi_refusals
from tests import connections_model as cm
from tests import connections_scenes as sc
from tests.abi_refusals import both, put

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY, COUNT, TARGETS, TARGETS_COUNT = "msl_connections_apply", 21, "msl_fuse_targets", 15


def test_exported_declared_and_bound():
    from manhattanslam_amd import _header, _lib
    dll = C.CDLL(_lib.LIB_PATH)
    decl = _header.declarations(_header.text("msl.h"))
    for entry, count in ((ENTRY, COUNT), (TARGETS, TARGETS_COUNT)):
        for n in (entry, entry + "_batch"):
            assert decl[n][0] == "int" and hasattr(dll, n), n
            res, args = _lib.SIGNATURES[n]
            assert res is C.c_int and len(args) == len(decl[n][1]) == count, n
            assert getattr(_lib.lib, n).argtypes == args
        a, b = decl[entry][1], decl[entry + "_batch"][1]
        assert a[0] == ("msl_match *", "h") and b[0] == ("int", "device") and a[1:] == b[1:]
    assert _lib.RECORDS["msl_conn_op"].names == ("op", "a", "b", "c") and _lib.RECORDS["msl_conn_op"].itemsize == 16


def test_argument_order_codes_and_limits_are_the_wrapper_s_and_the_model_s():
    import manhattanslam_amd as m
    from manhattanslam_amd import _header, connections as cn
    assert m.connections is cn and all(callable(getattr(cn, n)) for n in cn.__all__ if n[0].islower())
    src = _header.text("msl.h")
    decl = _header.declarations(src)
    names = [x[1] for x in decl[ENTRY][1]]
    assert names[1:8] == ["n_tab", "ccap", "n_rows", "n_ops", "tcap", "origin", "th"] and tuple(names[8:10]) == cn.IN_KEYS
    assert tuple(names[10:16]) == cn.INOUT_KEYS and names[16] == "mem" and tuple(names[17:20]) == cn.OUT_KEYS and names[20] == "out_mem"
    names = [x[1] for x in decl[TARGETS][1]]
    assert names[1:7] == ["n_tab", "ccap", "n_items", "nn", "nn2", "tcap"] and tuple(names[7:11]) == cn.TARGETS_IN_KEYS
    assert names[11] == "mem" and tuple(names[12:14]) == cn.TARGETS_OUT_KEYS and names[14] == "out_mem"
    define = lambda n: int(re.search(r"#define\s+%s\s+(\d+)\b" % n, src).group(1))
    for mod in (cn, cm):
        assert [define("MSL_CONN_" + n) for n in ("UPDATE", "KF_BAD", "MAX_OPS")] == [mod.UPDATE, mod.KF_BAD, mod.MAX_OPS]
        assert [define("MSL_CONN_" + n) for n in ("DONE", "PARENT_SET", "EMPTY", "ALREADY_BAD", "KEPT")] == \
            [mod.DONE, mod.PARENT_SET, mod.EMPTY, mod.ALREADY_BAD, mod.KEPT]
        assert (mod.LIVE, mod.NOT_ERASE, mod.CONNECTED) == (1, 2, 4)
    text = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", "msl.h")).read())
    line = re.search(r"Limits: n_tab <= (\d+), 1 <= ccap <= n_tab, 0 <= n_rows <= n_tab, 1 <= n_ops <= (\d+), 1 <= tcap <= n_tab", text)
    assert tuple(int(x) for x in line.groups()) == (cn.MAX_TAB, cn.MAX_OPS) == (cm.MAX_TAB, cm.MAX_OPS)
    assert "bit 0: !isBad(); bit 1: mbNotErase; bit 2: !mbFirstConnection" in text


def test_shared_arrays_have_the_names_and_types_of_the_other_entries():
    from manhattanslam_amd import _header
    decl = _header.declarations(_header.text("msl.h"))
    mine = {n: t for t, n in decl[ENTRY][1]}
    targets = {n: t for t, n in decl[TARGETS][1]}
    covis = {n: t for t, n in decl["msl_covisibility"][1]}
    local = {n: t for t, n in decl["msl_local_keyframes"][1]}
    cand = {n: t for t, n in decl["msl_fuse_candidates"][1]}
    for k in ("conn", "conn_w", "n_conn"):                                # written there and here
        assert mine[k] == covis[k] and not mine[k].startswith("const"), k
    assert mine["weight"] == "const " + covis["weight"]                   # msl_covisibility's output is this entry's input
    for k in ("conn", "n_conn", "parent", "kf_flags"):                    # in place here: the readers' type without its const
        assert "const " + mine[k] == local[k], k
    for k in ("conn", "n_conn", "kf_flags"):
        assert targets[k] == local[k], k
    for k in ("targets", "n_targets"):                                    # msl_fuse_targets' outputs are msl_fuse_candidates' inputs
        assert "const " + targets[k] == cand[k], k
    assert {mine[k] for k in ("ccap", "th")} == {covis[k] for k in ("ccap", "th")} == {"int"} and targets["tcap"] == cand["tcap"]


# ---- refusals of msl_connections_apply -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    s = sc.pin_early_returns()
    a, sh = sc.pack(s)
    assert sh == dict(n_tab=5, ccap=5, n_rows=2, n_ops=7, tcap=5, origin=0, th=15) and {o[0] for o in s["ops"]} == {cm.UPDATE, cm.KF_BAD}
    assert a["n_conn"].tolist() == [2, 2, 2, 2, 2] and s["ops"][4][:2] == (cm.UPDATE, 2)
    return a, sh


def op(o, field, value):
    """The edit ops[o].field = value."""
    def edit(x):
        x[field][o] = value
    return edit


def at(row, col, value):
    def edit(x):
        x[row][col] = value
    return edit


def refused(scene, **over):
    from manhattanslam_amd import connections as cn
    a, sh = scene
    return abi_refusals.refused(ENTRY, sh, a, cn.outputs(sh["n_ops"], sh["tcap"], sc.host_filled), inout=cn.INOUT_KEYS, **over)


LIMITS = both("n_tab", 4096) + both("ccap", 5, "n_tab = 5") + both("n_ops", 4096) + both("tcap", 5, "n_tab = 5") + \
    [("n_rows", -1, "n_rows -1 outside 0 .. n_tab = 5"), ("n_rows", 6, "n_rows 6 outside 0 .. n_tab = 5"), ("n_rows", 0, "weight is given while n_rows is 0"),
     ("origin", -2, "origin is keyframe -2 of 5"), ("origin", 5, "origin is keyframe 5 of 5"), ("th", 0, "th 0 below 1"), ("th", -15, "th -15 below 1")]


def test_every_limit_is_refused_with_the_field_named(scene):
    assert {l[0] for l in LIMITS} == set(abi_refusals.declared(ENTRY)[0])
    for field, value, msg in LIMITS:
        assert refused(scene, **{field: value}) == f"{ENTRY}: {msg}"


def test_every_null_is_refused_with_the_field_named(scene):
    pointers = abi_refusals.declared(ENTRY)[1]
    assert len(pointers) == 11
    for n in pointers:
        assert refused(scene, **{n: None}) == f"{ENTRY}: {n} is NULL"


def test_weight_is_null_exactly_when_there_are_no_rows(scene):
    """A log of KF_BAD alone needs no weight row: accepted checks are not part of this file (a launch), the refusals around it are."""
    a, sh = scene
    assert refused(scene, weight=None, n_rows=0) == f"{ENTRY}: ops[4].b is weight row 0 of 0"      # the UPDATE ops name a row


def test_index_defects_of_a_host_memory_call_are_refused(scene):
    e = ENTRY
    assert refused(scene, ops=op(0, "op", 0)) == f"{e}: ops[0].op is 0, not an MSL_CONN_* code"
    assert refused(scene, ops=op(6, "op", 3)) == f"{e}: ops[6].op is 3, not an MSL_CONN_* code"
    assert refused(scene, ops=op(1, "a", 5)) == f"{e}: ops[1].a is keyframe 5 of 5"
    assert refused(scene, ops=op(4, "a", -1)) == f"{e}: ops[4].a is keyframe -1 of 5"
    assert refused(scene, ops=op(4, "b", 2)) == f"{e}: ops[4].b is weight row 2 of 2"
    assert refused(scene, ops=op(5, "b", -1)) == f"{e}: ops[5].b is weight row -1 of 2"
    assert refused(scene, n_conn=put(3, -1)) == f"{e}: n_conn[3] is -1 outside 0 .. n_tab = 5"
    assert refused(scene, n_conn=put(3, 6)) == f"{e}: n_conn[3] is 6 outside 0 .. n_tab = 5"
    assert refused(scene, conn=at(2, 1, 5)) == f"{e}: conn[2][1] is keyframe 5 of 5"
    assert refused(scene, conn=at(4, 0, -1)) == f"{e}: conn[4][0] is keyframe -1 of 5"
    assert refused(scene, parent=put(1, -2)) == f"{e}: parent[1] is keyframe -2 of 5"
    assert refused(scene, parent=put(4, 5)) == f"{e}: parent[4] is keyframe 5 of 5"
    assert refused(scene, weight=at(1, 4, -9)) == f"{e}: weight[1][4] is -9, below 0"
    assert refused(scene, cw=at(3, 0, -1)) == f"{e}: cw[3][0] is -1, below 0"


def test_the_handle_forms_refuse_a_null_handle():
    from manhattanslam_amd import _lib
    for entry, count in ((ENTRY, COUNT), (TARGETS, TARGETS_COUNT)):
        args = [0 if t in (C.c_int, C.c_uint) else None for t in _lib.SIGNATURES[entry][1][1:]]
        assert len(args) == count - 1 and getattr(_lib.lib, entry)(None, *args) == -1
        assert _lib.lib.msl_last_error().decode() == f"{entry}: h is NULL"


# ---- refusals of msl_fuse_targets ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def graph():
    st = sc.pin_early_returns()["state"]
    a = dict(conn=st["conn"], n_conn=st["n_conn"], kf_flags=st["kf_flags"], cur=np.array([4, 0, 2], np.int32))
    return a, dict(n_tab=5, ccap=5, n_items=3, nn=3, nn2=2, tcap=4)


def targets_refused(graph, **over):
    from manhattanslam_amd import connections as cn
    a, sh = graph
    return abi_refusals.refused(TARGETS, sh, a, cn.targets_outputs(sh["n_items"], sh["tcap"], sc.host_filled), **over)


TARGETS_LIMITS = both("n_tab", 4096) + both("ccap", 5, "n_tab = 5") + both("nn", 5, "n_tab = 5") + both("nn2", 5, "n_tab = 5") + \
    both("n_items", 5, "n_tab = 5") + both("tcap", 4096)


def test_fuse_targets_refuses_every_limit_null_and_index_defect(graph):
    ints, pointers = abi_refusals.declared(TARGETS)
    assert {l[0] for l in TARGETS_LIMITS} == set(ints) and len(pointers) == 6
    for field, value, msg in TARGETS_LIMITS:
        assert targets_refused(graph, **{field: value}) == f"{TARGETS}: {msg}"
    for n in pointers:
        assert targets_refused(graph, **{n: None}) == f"{TARGETS}: {n} is NULL"
    assert targets_refused(graph, n_conn=put(0, 6)) == f"{TARGETS}: n_conn[0] is 6 outside 0 .. n_tab = 5"
    assert targets_refused(graph, conn=at(1, 1, 5)) == f"{TARGETS}: conn[1][1] is keyframe 5 of 5"
    assert targets_refused(graph, cur=put(2, 5)) == f"{TARGETS}: cur[2] is 5 of 5"
    assert targets_refused(graph, cur=put(0, -1)) == f"{TARGETS}: cur[0] is -1 of 5"

"""CPU-only: the derived-cursor calls (include/aclgpu.h "derived lookup cursors") on a store-only engine.  The symbols are exported, the three records have the
header's sizes, the Python wrappers exist, and every refusal of an argument is answered before the engine's mode is looked at: only a well-formed call
reaches "no GPU here"."""
import ctypes as C

import numpy as np
import pytest

SCHEMA = "definition user {}\ndefinition group { relation member: user | group#member }\ndefinition doc { relation viewer: user | group#member\n permission view = viewer }"
NEW_SYMBOLS = ("acl_lookup_cursor_open_mixed", "acl_lookup_cursor_derive", "acl_lookup_cursor_count", "acl_lookup_derive_stats")


@pytest.fixture(scope="module")
def aclgpu(aclgpu_lib):
    import aclgpu as m
    return m


@pytest.fixture()
def eng(aclgpu):
    e = aclgpu.Engine(SCHEMA, store_only=True)
    e.touch(("doc", "d", "viewer", "user", "u", ""))
    yield e
    e.close()


def last_error(e):
    return (e._L.acl_last_error() or b"").decode()


def test_symbols_structs_and_wrappers(aclgpu, aclgpu_lib, tmp_path):
    import os
    import subprocess
    from aclgpu import _lib
    for sym in NEW_SYMBOLS:
        assert hasattr(aclgpu_lib, sym) and sym in _lib.SYMBOLS, sym
    assert C.sizeof(_lib.SubjectRef) == 16 and [f for f, _t in _lib.SubjectRef._fields_] == ["stype", "srel", "id", "reserved"]
    assert C.sizeof(_lib.RowRef) == 8 and [f for f, _t in _lib.RowRef._fields_] == ["cursor", "row"]
    assert C.sizeof(_lib.RowExpr) == 16 and [f for f, _t in _lib.RowExpr._fields_] == ["first", "n_any", "n_all", "n_none"]
    assert aclgpu.engine.SUBJECT_REF_DTYPE.itemsize == 16 and aclgpu.DERIVE_ANY_REVISION == 1
    # the header's own view of the three records (gcc), field by field
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    pairs = {"acl_subject_ref_t": _lib.SubjectRef, "acl_row_ref_t": _lib.RowRef, "acl_row_expr_t": _lib.RowExpr}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "aclgpu.h"', 'int main(void) {']
    for cname, ct in pairs.items():
        lines.append(f'printf("{cname} %zu", sizeof({cname}));')
        lines += [f'printf(" %zu", offsetof({cname}, {f}));' for f, _t in ct._fields_]
        lines.append('printf("\\n");')
    lines.append('printf("flag %u\\n", ACL_DERIVE_ANY_REVISION); return 0; }')
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-I", inc, "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")])
    out = dict((ln.split()[0], [int(x) for x in ln.split()[1:]]) for ln in subprocess.check_output([str(tmp_path / "layout")]).decode().splitlines())
    assert out["flag"] == [1]
    for cname, ct in pairs.items():
        assert out[cname] == [C.sizeof(ct)] + [getattr(ct, f).offset for f, _t in ct._fields_], cname
    for name in ("lookup_cursor_mixed", "derive_cursor", "count_rows", "principal_cursor"):
        assert callable(getattr(aclgpu.Engine, name)), name


def test_open_mixed_refuses_arguments_first_then_the_mode(aclgpu, eng):
    e, L = eng, eng._L
    doc, user, group = e.type_id("doc"), e.type_id("user"), e.type_id("group")
    view, member = e.relation_id("doc", "view"), e.relation_id("group", "member")
    out = C.c_void_p()

    def subj(rows):
        return np.array(rows, dtype=aclgpu.engine.SUBJECT_REF_DTYPE)

    def call(h, rt, pm, arr, n, outp):
        return L.acl_lookup_cursor_open_mixed(h, rt, pm, arr.ctypes.data if arr is not None else None, n, None, outp)

    ok = subj([(user, -1, 0, 0), (group, member, 0, 0)])
    assert call(e._h, doc, view, ok, 2, None) == aclgpu.ERR_INVALID_ARGUMENT and "NULL" in last_error(e)
    assert call(e._h, doc, view, None, 2, C.byref(out)) == aclgpu.ERR_INVALID_ARGUMENT and "NULL" in last_error(e)
    assert call(None, doc, view, ok, 2, C.byref(out)) == aclgpu.ERR_INVALID_ARGUMENT
    assert call(e._h, doc, view, subj([(user, -1, 0, 0), (user, -1, 0, 9)]), 2, C.byref(out)) == aclgpu.ERR_INVALID_ARGUMENT and "subject 1: reserved" in last_error(e)
    # a malformed subject is refused before an unknown type is
    assert call(e._h, 99, view, subj([(user, -1, 0, 1)]), 1, C.byref(out)) == aclgpu.ERR_INVALID_ARGUMENT
    # unknown type, permission or relation -- of the call, or of any one subject
    for rt, pm, rows in ((99, view, [(user, -1, 0, 0)]), (doc, 99, [(user, -1, 0, 0)]), (doc, -1, [(user, -1, 0, 0)]), (doc, view, [(99, -1, 0, 0)]),
                         (doc, view, [(user, -1, 0, 0), (user, 5, 0, 0)]), (doc, view, [(user, -1, 0, 0), (group, member + 1, 0, 0)]), (doc, view, [(user, -2, 0, 0)]),
                         (99, view, [])):
        out.value = 1
        assert call(e._h, rt, pm, subj(rows) if rows else None, len(rows), C.byref(out)) == aclgpu.ERR_FAILED_PRECONDITION, (rt, pm, rows)
        assert not out.value
    # a valid open: only now the mode
    for rows in ([(user, -1, 0, 0), (group, member, 0, 0), (user, -1, 0, 0)], []):
        assert call(e._h, doc, view, subj(rows) if rows else None, len(rows), C.byref(out)) == aclgpu.ERR_UNAVAILABLE
        assert "store-only" in last_error(e) and not out.value
    with pytest.raises(aclgpu.AclError) as ei:
        e.lookup_cursor_mixed("doc", "view", [("user", "", 0), ("group", "member", 0)])
    assert ei.value.code == aclgpu.ERR_UNAVAILABLE
    with pytest.raises(aclgpu.AclError) as ei:
        e.lookup_cursor_mixed("doc", "view", [("user", "nosuch", 0)])
    assert ei.value.code == aclgpu.ERR_FAILED_PRECONDITION
    with pytest.raises(aclgpu.AclError) as ei:
        e.principal_cursor("doc", "view", [[("user", "", "u"), ("group", "member", "g")]])
    assert ei.value.code == aclgpu.ERR_UNAVAILABLE


def test_derive_and_count_refuse_arguments_first_then_the_mode(aclgpu, eng):
    """no cursor can be open on a store-only engine: every source pointer is foreign.  The call's own fields are looked at first -- the message says which --
    then the pointers, and only a call without sources and expressions (the one well-formed call there is) reaches the engine's mode."""
    e, L = eng, eng._L
    foreign = C.c_void_p(0x1000)
    srcs = (C.c_void_p * 2)(foreign, foreign)
    out = C.c_void_p()
    counts = np.zeros(4, dtype=np.uint64)

    def u32(rows, width):
        return np.array(rows, dtype=np.uint32).reshape(-1, width)

    def derive(refs, exprs, flags=0, srcs_p=srcs, n_srcs=2):
        return L.acl_lookup_cursor_derive(e._h, srcs_p, n_srcs, refs.ctypes.data if refs is not None else None, 0 if refs is None else len(refs),
                                          exprs.ctypes.data if exprs is not None else None, 0 if exprs is None else len(exprs), flags, C.byref(out))

    def count(refs, exprs, flags=0, srcs_p=srcs, n_srcs=2, counts_p=counts.ctypes.data):
        return L.acl_lookup_cursor_count(e._h, srcs_p, n_srcs, refs.ctypes.data if refs is not None else None, 0 if refs is None else len(refs),
                                         exprs.ctypes.data if exprs is not None else None, 0 if exprs is None else len(exprs), flags, counts_p)

    refs, exprs = u32([[0, 0], [1, 0]], 2), u32([[0, 1, 0, 1]], 4)
    for fn in (derive, count):
        # NULL pointers
        assert fn(refs, exprs, srcs_p=None) == aclgpu.ERR_INVALID_ARGUMENT and "NULL" in last_error(e)
        assert fn(refs, exprs, srcs_p=(C.c_void_p * 2)(foreign, None)) == aclgpu.ERR_INVALID_ARGUMENT and "NULL" in last_error(e)
        assert L.acl_lookup_cursor_derive(e._h, srcs, 2, None, 2, exprs.ctypes.data, 1, 0, C.byref(out)) == aclgpu.ERR_INVALID_ARGUMENT and "NULL" in last_error(e)
        assert L.acl_lookup_cursor_count(e._h, srcs, 2, refs.ctypes.data, 2, None, 1, 0, counts.ctypes.data) == aclgpu.ERR_INVALID_ARGUMENT and "NULL" in last_error(e)
        # the call's own fields
        assert fn(refs, exprs, flags=2) == aclgpu.ERR_INVALID_ARGUMENT and "flag" in last_error(e)
        assert fn(refs, exprs, flags=0x80000001) == aclgpu.ERR_INVALID_ARGUMENT and "flag" in last_error(e)
        assert fn(u32([[0, 0], [2, 0]], 2), exprs) == aclgpu.ERR_INVALID_ARGUMENT and "ref 1: cursor 2" in last_error(e)
        assert fn(refs, u32([[0, 1, 0, 1], [1, 1, 1, 0]], 4)) == aclgpu.ERR_INVALID_ARGUMENT and "expression 1 runs past" in last_error(e)
        assert fn(refs, u32([[0xFFFFFFFF, 1, 0, 0]], 4)) == aclgpu.ERR_INVALID_ARGUMENT and "runs past" in last_error(e)
        assert fn(refs, u32([[0, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF]], 4)) == aclgpu.ERR_INVALID_ARGUMENT and "runs past" in last_error(e)
        assert fn(refs, u32([[0, 1, 0, 0], [0, 0, 0, 2]], 4)) == aclgpu.ERR_INVALID_ARGUMENT and "expression 1: n_any + n_all is 0" in last_error(e)
        # well-formed: now the pointers (a row beyond a cursor's rows needs the cursor: any row of a foreign pointer is refused with it)
        assert fn(refs, exprs) == aclgpu.ERR_INVALID_ARGUMENT and "not an open cursor" in last_error(e)
        assert fn(refs, exprs, flags=aclgpu.DERIVE_ANY_REVISION) == aclgpu.ERR_INVALID_ARGUMENT and "not an open cursor" in last_error(e)
        assert fn(None, None) == aclgpu.ERR_INVALID_ARGUMENT and "not an open cursor" in last_error(e)  # (sources nobody references are sources all the same)
        # no sources, no expressions: the mode
        assert fn(None, None, srcs_p=None, n_srcs=0) == aclgpu.ERR_UNAVAILABLE and "store-only" in last_error(e)
        assert fn(None, None, srcs_p=None, n_srcs=0, flags=4) == aclgpu.ERR_INVALID_ARGUMENT
    assert L.acl_lookup_cursor_derive(e._h, srcs, 2, refs.ctypes.data, 2, exprs.ctypes.data, 1, 0, None) == aclgpu.ERR_INVALID_ARGUMENT and "NULL" in last_error(e)
    assert count(refs, exprs, counts_p=None) == aclgpu.ERR_INVALID_ARGUMENT and "NULL" in last_error(e)
    assert L.acl_lookup_cursor_derive(None, None, 0, None, 0, None, 0, 0, C.byref(out)) == aclgpu.ERR_INVALID_ARGUMENT
    assert L.acl_lookup_cursor_count(None, None, 0, None, 0, None, 0, 0, None) == aclgpu.ERR_INVALID_ARGUMENT
    assert not out.value and not counts.any()
    # the Python wrappers, around a foreign handle and around nothing
    cur = aclgpu.LookupCursor(e, foreign, "doc", 1)
    for call in (lambda: e.derive_cursor([cur], [([(0, 0)], [], [])]), lambda: e.count_rows([cur, cur], [([(0, 0)], [(1, 0)], [])])):
        with pytest.raises(aclgpu.AclError) as ei:
            call()
        assert ei.value.code == aclgpu.ERR_INVALID_ARGUMENT
    for call in (lambda: e.derive_cursor([], []), lambda: e.count_rows([], [])):
        with pytest.raises(aclgpu.AclError) as ei:
            call()
        assert ei.value.code == aclgpu.ERR_UNAVAILABLE


def test_the_derive_counters(aclgpu):
    e = aclgpu.Engine(SCHEMA, store_only=True)
    st = e.stats()
    assert st["derive_launches"] == 0 and st["derive_ms"] == 0.0
    e.stats_reset()
    assert e.stats()["derive_launches"] == 0
    launches = C.c_uint64(7)
    assert e._L.acl_lookup_derive_stats(e._h, C.byref(launches), None) == 0 and launches.value == 0
    assert e._L.acl_lookup_derive_stats(None, C.byref(launches), None) == aclgpu.ERR_INVALID_ARGUMENT
    from aclgpu._lib import Stats
    assert "derive_launches" not in [f for f, _t in Stats._fields_]  # (like the page counters: not a field of acl_stats_t)
    e.close()

"""CPU-only: the lookup cursor calls (include/aclgpu.h "paged lookups") on a store-only engine.  Every argument refusal is answered before the engine's mode is
looked at -- NULL pointers, unknown types, the requests' own fields, a pointer that is no open cursor -- and only a valid open reaches "no GPU here"."""
import ctypes as C

import numpy as np
import pytest

SCHEMA = "definition user {}\ndefinition group { relation member: user | group#member }\ndefinition doc { relation viewer: user | group#member\n permission view = viewer }"


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


def open_raw(e, fn, rt, pm, st, sr, ids, out):
    arr = np.ascontiguousarray(ids, dtype=np.uint32)
    return fn(e._h, rt, pm, st, sr, arr.ctypes.data if ids is not None else None, 0 if ids is None else arr.size, None, out)


def test_open_refuses_arguments_first_then_the_mode(aclgpu, eng):
    e, L = eng, eng._L
    doc, user, group = e.type_id("doc"), e.type_id("user"), e.type_id("group")
    view, member = e.relation_id("doc", "view"), e.relation_id("group", "member")
    out = C.c_void_p()
    for fn in (L.acl_lookup_cursor_open, L.acl_lookup_cursor_open_subjects):
        # NULL pointers
        assert fn(e._h, doc, view, user, -1, np.zeros(1, dtype=np.uint32).ctypes.data, 1, None, None) == aclgpu.ERR_INVALID_ARGUMENT
        assert fn(e._h, doc, view, user, -1, None, 1, None, C.byref(out)) == aclgpu.ERR_INVALID_ARGUMENT
        assert fn(None, doc, view, user, -1, None, 0, None, C.byref(out)) == aclgpu.ERR_INVALID_ARGUMENT
        # unknown type, permission or relation
        for rt, pm, st, sr in ((99, view, user, -1), (-1, view, user, -1), (doc, 99, user, -1), (doc, -1, user, -1), (doc, view, 99, -1), (doc, view, user, 5),
                               (doc, view, user, -2), (doc, view, group, member + 1)):
            out.value = 1
            assert open_raw(e, fn, rt, pm, st, sr, [0], C.byref(out)) == aclgpu.ERR_FAILED_PRECONDITION, (rt, pm, st, sr)
            assert not out.value
        # a valid open: only now the mode
        for st, sr, ids in ((user, -1, [0]), (group, member, [0]), (user, -1, [])):
            assert open_raw(e, fn, doc, view, st, sr, ids, C.byref(out)) == aclgpu.ERR_UNAVAILABLE
            assert "store-only" in last_error(e) and not out.value
    for call in (lambda: e.lookup_cursor("doc", "view", "user", "", [0]), lambda: e.subjects_cursor("doc", "view", "user", "", [0])):
        with pytest.raises(aclgpu.AclError) as ei:
            call()
        assert ei.value.code == aclgpu.ERR_UNAVAILABLE
    with pytest.raises(aclgpu.AclError) as ei:
        e.lookup_cursor("doc", "view", "user", "nosuch", [0])
    assert ei.value.code == aclgpu.ERR_FAILED_PRECONDITION


def reqs_of(rows):
    return np.array(rows, dtype=np.uint32).reshape(-1, 4)


def test_pages_refuses_its_requests_before_it_looks_for_the_cursor(aclgpu, eng):
    """no cursor can be open on a store-only engine: the pointer is foreign.  The requests' own fields are looked at first -- the message says which."""
    e, L = eng, eng._L
    foreign = C.c_void_p(0x1000)
    ids, n, more = np.zeros(16, dtype=np.uint32), np.zeros(4, dtype=np.uint32), np.zeros(4, dtype=np.uint8)

    def pages(cur, reqs, m, ids_p, cap, n_p=n.ctypes.data, more_p=more.ctypes.data):
        return L.acl_lookup_cursor_pages(e._h, cur, reqs.ctypes.data if reqs is not None else None, m, ids_p, cap, n_p, more_p, None)

    ok = reqs_of([[0, aclgpu.PAGE_FROM_START, 4, 0]])
    assert pages(None, ok, 1, ids.ctypes.data, 16) == aclgpu.ERR_INVALID_ARGUMENT and "NULL" in last_error(e)
    assert pages(foreign, None, 1, ids.ctypes.data, 16) == aclgpu.ERR_INVALID_ARGUMENT and "NULL" in last_error(e)
    assert pages(foreign, ok, 1, ids.ctypes.data, 16, n_p=None) == aclgpu.ERR_INVALID_ARGUMENT and "NULL" in last_error(e)
    assert pages(foreign, ok, 1, ids.ctypes.data, 16, more_p=None) == aclgpu.ERR_INVALID_ARGUMENT and "NULL" in last_error(e)
    assert pages(foreign, ok, 1, None, 16) == aclgpu.ERR_INVALID_ARGUMENT
    assert pages(foreign, reqs_of([[0, 0, 4, 0], [0, 0, 0, 0]]), 2, ids.ctypes.data, 16) == aclgpu.ERR_INVALID_ARGUMENT and "request 1: limit is 0" in last_error(e)
    assert pages(foreign, reqs_of([[0, 0, 4, 7]]), 1, ids.ctypes.data, 16) == aclgpu.ERR_INVALID_ARGUMENT and "reserved" in last_error(e)
    assert pages(foreign, reqs_of([[0, 0, 4, 0], [0, 0, 13, 0]]), 2, ids.ctypes.data, 16) == aclgpu.ERR_INVALID_ARGUMENT and "fewer ids than the limits" in last_error(e)
    assert pages(foreign, reqs_of([[0, 0, 1 << 28, 0], [0, 0, 1, 0]]), 2, ids.ctypes.data, 1 << 30) == aclgpu.ERR_INVALID_ARGUMENT and "2^28" in last_error(e)
    # well-formed requests: now the pointer (row >= n needs a cursor: any row of a foreign pointer is refused with it)
    assert pages(foreign, ok, 1, ids.ctypes.data, 16) == aclgpu.ERR_INVALID_ARGUMENT and "not an open cursor" in last_error(e)
    assert pages(foreign, reqs_of([[5, 0, 4, 0]]), 1, ids.ctypes.data, 16) == aclgpu.ERR_INVALID_ARGUMENT
    assert pages(foreign, ok, 0, None, 0, n_p=None, more_p=None) == aclgpu.ERR_INVALID_ARGUMENT and "not an open cursor" in last_error(e)
    assert not ids.any() and not n.any() and not more.any()


def test_the_other_calls_refuse_a_foreign_or_closed_cursor(aclgpu, eng):
    e, L = eng, eng._L
    foreign = C.c_void_p(0x1000)
    rev, nr, rt = C.c_uint64(), C.c_uint32(), C.c_uint32()
    assert L.acl_lookup_cursor_info(e._h, foreign, C.byref(rev), C.byref(nr), C.byref(rt), None, None) == aclgpu.ERR_INVALID_ARGUMENT
    assert L.acl_lookup_cursor_info(e._h, None, C.byref(rev), C.byref(nr), C.byref(rt), None, None) == aclgpu.ERR_INVALID_ARGUMENT
    assert L.acl_lookup_cursor_close(e._h, foreign) == aclgpu.ERR_INVALID_ARGUMENT and "not an open cursor" in last_error(e)
    assert L.acl_lookup_cursor_close(e._h, None) == aclgpu.ERR_INVALID_ARGUMENT
    assert L.acl_lookup_cursor_close(None, foreign) == aclgpu.ERR_INVALID_ARGUMENT
    ids, ends, buf = np.zeros(4, dtype=np.uint32), np.zeros(4, dtype=np.uint32), C.create_string_buffer(2048)
    n, more = C.c_uint32(), C.c_uint8()

    def names(cur, limit=4, ids_p=ids.ctypes.data, cap=2048, ends_p=ends.ctypes.data):
        return L.acl_lookup_cursor_page_names(e._h, cur, 0, aclgpu.PAGE_FROM_START, limit, ids_p, buf, cap, ends_p, C.byref(n), C.byref(more))

    assert names(foreign) == aclgpu.ERR_INVALID_ARGUMENT and "not an open cursor" in last_error(e)
    assert names(foreign, limit=0) == aclgpu.ERR_INVALID_ARGUMENT and "limit is 0" in last_error(e)
    assert names(foreign, ids_p=None) == aclgpu.ERR_INVALID_ARGUMENT
    assert names(foreign, ends_p=None) == aclgpu.ERR_INVALID_ARGUMENT
    assert names(foreign, cap=100) == aclgpu.ERR_INVALID_ARGUMENT and "1024" in last_error(e)
    assert names(None) == aclgpu.ERR_INVALID_ARGUMENT
    # the Python wrapper: a cursor object around a closed handle
    cur = aclgpu.LookupCursor(e, foreign, "doc", 1)
    for call in (cur.info, lambda: cur.page(0, limit=4), lambda: cur.pages([(0, None, 2), (0, 5, 2)]), lambda: cur.page_names(0, None, 4), cur.close):
        with pytest.raises(aclgpu.AclError) as ei:
            call()
        assert ei.value.code == aclgpu.ERR_INVALID_ARGUMENT


def test_close_with_nothing_open_and_the_page_counters(aclgpu):
    e = aclgpu.Engine(SCHEMA, store_only=True)
    st = e.stats()
    assert st["page_launches"] == 0 and st["page_ms"] == 0.0
    e.stats_reset()
    assert e.stats()["page_launches"] == 0
    e.close()  # (acl_close walks an empty list of cursors)
    from aclgpu._lib import PageReq
    assert C.sizeof(PageReq) == 16 and [f for f, _t in PageReq._fields_] == ["row", "after_id", "limit", "reserved"]

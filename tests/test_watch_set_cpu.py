"""Watch sets without a GPU: the entry points are exported and bound, a store-only engine refuses to open a set (there is no CPU evaluation path),
and bad arguments are refused with the codes include/aclgpu.h lists."""
import ctypes as C

import numpy as np
import pytest

SCHEMA = "definition user {}\ndefinition group { relation member: user }\ndefinition doc { relation viewer: user | group#member\n permission view = viewer }"
NAMES = ["acl_watch_set_open", "acl_watch_set_add", "acl_watch_set_remove", "acl_watch_set_poll", "acl_watch_set_row", "acl_watch_set_stats", "acl_watch_set_close",
         "acl_selfcheck_rows_diff"]


@pytest.fixture(scope="module")
def aclgpu(aclgpu_lib):
    import aclgpu as m
    return m


def test_symbols_are_exported_and_bound(aclgpu, aclgpu_lib):
    for n in NAMES:
        assert hasattr(aclgpu_lib, n) and n in aclgpu._lib.SYMBOLS, n
    assert aclgpu.WATCH_CHANGE_DTYPE.itemsize == C.sizeof(aclgpu._lib.WatchChange) == 16
    assert [f for f, _t in aclgpu._lib.WatchChange._fields_] == list(aclgpu.WATCH_CHANGE_DTYPE.names) == ["watcher", "resource_id", "gained", "reserved"]
    assert aclgpu.WATCHER_FROM_NOW == 1


def test_store_only_engine_refuses_a_watch_set(aclgpu):
    with aclgpu.Engine(SCHEMA, store_only=True) as e:
        e.touch(("doc", "d", "viewer", "user", "u", ""))
        for srel_args in (("user",), ("group", "member")):
            with pytest.raises(aclgpu.AclError) as ei:
                e.watch_set("doc", "view", *srel_args)
            assert ei.value.code == aclgpu.ERR_UNAVAILABLE
        with pytest.raises(aclgpu.AclError) as ei:  # the diff kernels' test hook needs the device too
            e.selfcheck_rows_diff(np.zeros((1, 4), dtype=np.uint32), np.ones((1, 4), dtype=np.uint32))
        assert ei.value.code == aclgpu.ERR_UNAVAILABLE


def test_bad_arguments_are_refused(aclgpu, aclgpu_lib):
    L = aclgpu_lib
    with aclgpu.Engine(SCHEMA, store_only=True) as e:
        # unknown type / permission / subject relation: FAILED_PRECONDITION (before the engine's kind is looked at)
        for args in (("nosuchtype", "view", "user"), ("doc", "nosuchperm", "user"), ("doc", "view", "nosuchtype"), ("doc", "view", "group", "nosuchrel")):
            with pytest.raises(aclgpu.AclError) as ei:
                e.watch_set(*args)
            assert ei.value.code == aclgpu.ERR_FAILED_PRECONDITION, args
        out = C.c_void_p()
        doc, user = e.type_id("doc"), e.type_id("user")
        assert L.acl_watch_set_open(e._h, doc, 99, user, -1, C.byref(out)) == aclgpu.ERR_FAILED_PRECONDITION and not out.value
        assert L.acl_watch_set_open(e._h, doc, e.relation_id("doc", "view"), user, -1, None) == aclgpu.ERR_INVALID_ARGUMENT
        # a handle that is no open set of this engine (NULL, or any other pointer): INVALID_ARGUMENT from every entry point, nothing is dereferenced
        w, n, rev, recs = C.c_uint32(), C.c_size_t(), C.c_uint64(), C.POINTER(aclgpu._lib.WatchChange)()
        bogus = C.c_void_p(0x1000)
        for s in (None, bogus):
            assert L.acl_watch_set_add(e._h, s, b"u", 0, C.byref(w)) == aclgpu.ERR_INVALID_ARGUMENT
            assert L.acl_watch_set_remove(e._h, s, 0) == aclgpu.ERR_INVALID_ARGUMENT
            assert L.acl_watch_set_poll(e._h, s, None, C.byref(recs), C.byref(n), C.byref(rev)) == aclgpu.ERR_INVALID_ARGUMENT
            assert L.acl_watch_set_row(e._h, s, 0, None, 0) == aclgpu.ERR_INVALID_ARGUMENT
            assert L.acl_watch_set_stats(e._h, s, None, None, None) == aclgpu.ERR_INVALID_ARGUMENT
            assert L.acl_watch_set_close(e._h, s) == aclgpu.ERR_INVALID_ARGUMENT
        assert b"watch set" in L.acl_last_error()
        assert L.acl_selfcheck_rows_diff(e._h, None, 4, None, 4, 1, C.byref(recs), C.byref(n)) == aclgpu.ERR_INVALID_ARGUMENT

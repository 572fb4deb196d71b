"""LookupSubjects on the sharded graph without a GPU: the two entry points exist, their ctypes bindings match the header, a store-only engine
refuses to evaluate, missing communicator callbacks are argument errors, and the Python client mirrors LookupSubjects."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "aclgpu.h")

SCHEMA = """
definition user {}
definition group {
  relation member: user | group#member
}
definition doc {
  relation viewer: user | user:* | group#member
  relation banned: user
  permission view = viewer - banned
}
"""


@pytest.fixture(scope="module")
def aclgpu(aclgpu_lib):
    import aclgpu as m
    return m


def _params(name):
    hdr = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", hdr, flags=re.S)
    assert m, name
    return [p for p in m.group(1).split(",") if p.strip()]


def test_bindings_match_the_header(aclgpu, aclgpu_lib):
    for name in ("acl_shard_subjects_bulk", "acl_shard_subjects_bulk_rccl"):
        assert name in aclgpu._lib.SYMBOLS and hasattr(aclgpu_lib, name)
        assert len(getattr(aclgpu_lib, name).argtypes) == len(_params(name)), name
    assert len(_params("acl_shard_subjects_bulk")) == 13 and len(_params("acl_shard_subjects_bulk_rccl")) == 12
    # the communicator is what the other native loops take
    assert aclgpu_lib.acl_shard_subjects_bulk.argtypes[1] == aclgpu_lib.acl_shard_lookup_bulk.argtypes[1]


def _comm(lib_mod, gather=True, reduce=True):
    called = []

    def all_gather(_u, _s, _r, _n, _st):
        called.append("gather")
        return 13

    def all_reduce(_u, _b, _n, _st):
        called.append("reduce")
        return 13

    cbs = (lib_mod.ALL_GATHER_CB(all_gather), lib_mod.ALL_REDUCE_CB(all_reduce))
    comm = lib_mod.ShardComm(None, cbs[0] if gather else lib_mod.ALL_GATHER_CB(), cbs[1] if reduce else lib_mod.ALL_REDUCE_CB(), lib_mod.ALL_TO_ALL_CB())
    return comm, cbs, called


def test_store_only_engine_and_missing_callbacks(aclgpu, aclgpu_lib):
    L = aclgpu._lib
    with aclgpu.Engine(SCHEMA, store_only=True) as e:
        e.touch(("doc", "d", "viewer", "user", "alice", ""), ("doc", "d", "viewer", "group", "g", "member"))
        rids = np.zeros(1, dtype=np.uint32)
        rows = np.zeros(4, dtype=np.uint32)  # (never written: every call below fails before it evaluates)
        st = L.ShardBulkStats()
        args = (e.type_id("doc"), e.relation_id("doc", "view"), e.type_id("user"), -1, rids.ctypes.data, 1, rows.ctypes.data, 4, None, None, C.byref(st))
        comm, keep, called = _comm(L)
        assert aclgpu_lib.acl_shard_subjects_bulk(e._h, C.byref(comm), *args) == aclgpu.ERR_UNAVAILABLE
        assert aclgpu_lib.acl_shard_subjects_bulk_rccl(e._h, *args) == aclgpu.ERR_UNAVAILABLE
        # NULL or missing callbacks: argument errors, before anything else
        assert aclgpu_lib.acl_shard_subjects_bulk(e._h, None, *args) == aclgpu.ERR_INVALID_ARGUMENT
        for gather, reduce in ((False, True), (True, False)):
            comm, keep, called2 = _comm(L, gather, reduce)
            assert aclgpu_lib.acl_shard_subjects_bulk(e._h, C.byref(comm), *args) == aclgpu.ERR_INVALID_ARGUMENT
            assert not called2
        assert not called
        # ... and so is a batch without buffers
        comm, keep, called = _comm(L)
        bad = args[:4] + (None, 1) + args[6:]
        assert aclgpu_lib.acl_shard_subjects_bulk(e._h, C.byref(comm), *bad) == aclgpu.ERR_INVALID_ARGUMENT
        with pytest.raises(aclgpu.AclError) as x:
            e._check(aclgpu_lib.acl_shard_subjects_bulk(e._h, C.byref(comm), *args))
        assert x.value.code == aclgpu.ERR_UNAVAILABLE and "store-only" in str(x.value)


def test_sharded_engine_has_the_method(aclgpu):
    from aclgpu import sharded
    sig = inspect.signature(sharded.ShardedEngine.lookup_subjects_ids_batch_native)
    assert list(sig.parameters)[1:] == ["rtype", "perm", "stype", "srel", "resource_ids", "want_excluded"]
    assert sig.parameters["want_excluded"].default is False


class _FakeEngine:
    """what PermissionsServiceClient.LookupSubjects needs of an Engine"""
    revision = 7

    def __init__(self, answer):
        self.answer, self.calls = answer, []

    def lookup_subjects(self, rt, rid, perm, st, srel=""):
        self.calls.append((rt, rid, perm, st, srel))
        return self.answer


def test_client_lookup_subjects_is_implemented():
    """PermissionsServiceClient.LookupSubjects is no longer the UNIMPLEMENTED stub: a stream of subject ids over Engine.lookup_subjects, `*` first
    with its excluded ids when the wildcard is set."""
    from aclgpu import client
    C_ = client.PermissionsServiceClient
    assert C_.LookupSubjects is not C_._unimplemented and C_.ExpandPermissionTree is C_._unimplemented
    req = client.LookupSubjectsRequest(client.ObjectReference("doc", "d"), "view", "user")
    fe = _FakeEngine(({"bob", "alice"}, False, set()))
    got = list(C_(fe).LookupSubjects(req))
    assert fe.calls == [("doc", "d", "view", "user", "")]
    assert [g.subject.subject_object_id for g in got] == ["alice", "bob"] and all(g.excluded_subjects == [] and g.looked_up_at == 7 for g in got)
    assert all(g.subject.permissionship == client.LOOKUP_PERMISSIONSHIP_HAS_PERMISSION for g in got)
    # a wildcard answer: `*` first, with the ids it leaves out
    fe = _FakeEngine(({"carol"}, True, {"u2", "u1"}))
    req = client.LookupSubjectsRequest(client.ObjectReference("doc", "d"), "view", "group", "member")
    got = list(C_(fe).LookupSubjects(req))
    assert fe.calls == [("doc", "d", "view", "group", "member")]
    assert [g.subject.subject_object_id for g in got] == ["*", "carol"]
    assert [x.subject_object_id for x in got[0].excluded_subjects] == ["u1", "u2"] and got[1].excluded_subjects == []
    assert all(x.permissionship != client.LOOKUP_PERMISSIONSHIP_HAS_PERMISSION for x in got[0].excluded_subjects)

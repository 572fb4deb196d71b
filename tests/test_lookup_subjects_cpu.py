"""LookupSubjects without a GPU: the entry points exist, their ctypes bindings match the header, and a store-only engine refuses to evaluate."""
import os
import re

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "aclgpu.h")


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
    for name in ("acl_lookup_subjects_batch", "acl_lookup_subjects"):
        assert name in aclgpu._lib.SYMBOLS and hasattr(aclgpu_lib, name)
        assert len(getattr(aclgpu_lib, name).argtypes) == len(_params(name)), name
    assert len(_params("acl_lookup_subjects_batch")) == 13 and len(_params("acl_lookup_subjects")) == 12


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


def test_store_only_engine_is_unavailable(aclgpu):
    with aclgpu.Engine(SCHEMA, store_only=True) as e:
        e.touch(("doc", "d", "viewer", "user", "alice", ""), ("doc", "d", "viewer", "group", "g", "member"))
        for call in (lambda: e.lookup_subjects("doc", "d", "view", "user"),
                     lambda: e.lookup_subjects("doc", "unknown-doc", "view", "user"),
                     lambda: e.lookup_subjects_ids_batch("doc", "view", "user", "", [0]),
                     lambda: e.lookup_subjects_ids_batch("doc", "view", "group", "member", [0], want_excluded=True)):
            with pytest.raises(aclgpu.AclError) as x:
                call()
            assert x.value.code == aclgpu.ERR_UNAVAILABLE
        # argument errors come first, as for LookupResources
        with pytest.raises(aclgpu.AclError) as x:
            e.lookup_subjects("doc", "not an id", "view", "user")
        assert x.value.code == aclgpu.ERR_INVALID_ARGUMENT
        with pytest.raises(aclgpu.AclError) as x:
            e.lookup_subjects("doc", "d", "nope", "user")
        assert x.value.code == aclgpu.ERR_FAILED_PRECONDITION

"""Explain for revocation without a GPU: the checker's own behaviour on hand cases (tests/revoke_checker.py must REJECT a missing cut, a surplus cut and a
relationship that is not stored), the refusals acl_explain_revoke* decides before an evaluation, on a store-only engine, and the ctypes prototypes against
the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import denial_checker as D
from tests import revoke_checker as R

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aclgpu.h")


@pytest.fixture(scope="module")
def aclgpu(aclgpu_lib):
    import aclgpu as m
    return m


# ---------------------------------------------------------------- the checker on hand cases
ITEM = ("doc", "d", "view", "user", "u", "")
CHAIN = [("doc", "d", "viewer", "group", "g", "member"), ("group", "g", "member", "group", "h", "member"), ("group", "h", "member", "user", "u", "")]
SIDE = [("group", "g", "member", "group", "k", "member"), ("group", "k", "member", "user", "u", ""), ("doc", "d", "owner", "user", "v", "")]


def test_checker_accepts_the_cuts_of_a_chain():
    ck = R.Checker(D.GROUPS, CHAIN + SIDE[2:])
    ck.check(ITEM, CHAIN, witness=CHAIN)
    ck.check(ITEM, list(reversed(CHAIN)))  # (a set: the order is not the checker's business)
    assert ck.brute([ITEM, ("doc", "d", "view", "user", "nobody", "")]) == {ITEM: frozenset(CHAIN)}


def test_checker_accepts_the_shared_hops_of_a_diamond():
    ck = R.Checker(D.GROUPS, CHAIN + SIDE)
    ck.check(ITEM, [CHAIN[0]], witness=CHAIN)
    ck.check(ITEM, [CHAIN[0]], witness=CHAIN, sample=2)


def test_checker_rejects_a_missing_cut():
    ck = R.Checker(D.GROUPS, CHAIN + SIDE[2:])
    with pytest.raises(AssertionError, match="is not listed"):
        ck.check(ITEM, CHAIN[:2], witness=CHAIN)
    with pytest.raises(AssertionError, match="is not listed"):
        ck.check(ITEM, [], witness=CHAIN)
    with pytest.raises(AssertionError, match="is not listed"):  # the sampled form still tries every hop of the witness
        ck.check(ITEM, CHAIN[:2], witness=CHAIN, sample=0)


def test_checker_rejects_a_surplus_cut():
    ck = R.Checker(D.GROUPS, CHAIN + SIDE)
    with pytest.raises(AssertionError, match="does not revoke"):
        ck.check(ITEM, [CHAIN[0], CHAIN[1]], witness=CHAIN)
    with pytest.raises(AssertionError, match="does not revoke"):  # stored, and nowhere near the item
        ck.check(ITEM, [CHAIN[0], SIDE[2]], witness=CHAIN)
    with pytest.raises(AssertionError, match="listed twice"):
        ck.check(ITEM, [CHAIN[0], CHAIN[0]], witness=CHAIN)


def test_checker_rejects_a_relationship_that_is_not_stored():
    ck = R.Checker(D.GROUPS, CHAIN)
    with pytest.raises(AssertionError, match="not a stored relationship"):
        ck.check(ITEM, CHAIN + [("doc", "d", "viewer", "user", "u", "")], witness=CHAIN)
    with pytest.raises(AssertionError, match="not granted"):
        ck.check(("doc", "d", "view", "user", "nobody", ""), [])


def test_checker_leaves_the_oracles_as_they_were():
    schema = D.GROUPS.replace("relation member: user | group#member", "relation member: user | group#member with expiration")
    ck = R.Checker(schema, {CHAIN[0]: 0, CHAIN[1]: 500, CHAIN[2]: 0}, now=100)
    ck.check(ITEM, CHAIN, witness=CHAIN)
    assert ck.orcs.c.num_tuples() == 3 and ck.granted(ITEM)
    ck.orcs.c.set_now(500)  # the expiry the probe put back is the one the relationship had
    assert ck.orcs.c.check(*ITEM)[0] != R.ORC_HAS


# ---------------------------------------------------------------- refusals decided before an evaluation
def raw_call(aclgpu, e, items, n, perm=True, off=True, cuts=True):
    """acl_explain_revoke_bulk_ids with any of its buffers left out -> (return code, offsets, the cuts pointer)"""
    L = aclgpu._lib.load()
    p = np.zeros(max(n, 1), dtype=np.uint8)
    o = np.full(n + 1, 7, dtype=np.uint32)
    cp = C.POINTER(aclgpu._lib.ExplainHop)()
    rc = L.acl_explain_revoke_bulk_ids(e._h, items.ctypes.data if items is not None else None, n, p.ctypes.data if perm else None, None, None,
                                       o.ctypes.data if off else None, C.byref(cp) if cuts else None, None)
    return rc, o, cp


def test_null_arguments_and_n_zero(aclgpu):
    e = aclgpu.Engine(D.GROUPS, store_only=True)
    e.touch(*CHAIN)
    items = e.make_items("doc", "view", [0], "user", "", [0])
    for kw in (dict(off=False), dict(cuts=False), dict(perm=False)):
        rc, _, _ = raw_call(aclgpu, e, items, 1, **kw)
        assert rc == aclgpu.ERR_INVALID_ARGUMENT and b"acl_explain_revoke_bulk_ids: NULL buffer" in aclgpu._lib.load().acl_last_error()
    assert raw_call(aclgpu, e, None, 1)[0] == aclgpu.ERR_INVALID_ARGUMENT
    # a store-only engine refuses before it looks at n, as acl_explain_bulk_ids does; its outputs were reset behind the NULL test
    rc, off, cp = raw_call(aclgpu, e, None, 0)
    assert rc == aclgpu.ERR_UNAVAILABLE and int(off[0]) == 0 and not cp
    L = aclgpu._lib.load()
    it = aclgpu._lib.CheckItem(b"doc", b"d", b"view", b"user", b"u", b"")
    p, er, txt = C.c_uint8(), C.c_int32(), C.c_void_p()
    for args in ((None, C.byref(p), C.byref(er), None, C.byref(txt)), (C.byref(it), None, C.byref(er), None, C.byref(txt)),
                 (C.byref(it), C.byref(p), None, None, C.byref(txt)), (C.byref(it), C.byref(p), C.byref(er), None, None)):
        assert L.acl_explain_revoke(e._h, *args, None) == aclgpu.ERR_INVALID_ARGUMENT and b"acl_explain_revoke: NULL argument" in L.acl_last_error()


def test_store_only_engine_refuses(aclgpu):
    e = aclgpu.Engine(D.GROUPS, store_only=True)
    e.touch(*CHAIN)
    with pytest.raises(aclgpu.AclError) as ei:
        e.explain_revoke_ids(e.make_items("doc", "view", [0], "user", "", [0]))
    assert ei.value.code == aclgpu.ERR_UNAVAILABLE
    with pytest.raises(aclgpu.AclError) as ei:
        e.explain_revoke(*ITEM)
    assert ei.value.code == aclgpu.ERR_UNAVAILABLE
    with pytest.raises(aclgpu.AclError) as ei:  # an invalid name in the string form: the API's validation comes first, as for acl_explain
        e.explain_revoke("doc", "d", "view", "user", "b*b")
    assert ei.value.code == aclgpu.ERR_INVALID_ARGUMENT
    with pytest.raises(aclgpu.AclError) as ei:
        e.explain_revoke("doc", "not an id", "view", "user", "u")
    assert ei.value.code == aclgpu.ERR_INVALID_ARGUMENT


def test_no_schema(aclgpu):
    bare = aclgpu.Engine(store_only=True)
    with pytest.raises(aclgpu.AclError) as ei:  # the string form interns the item first: no schema comes before the store-only refusal, as for acl_explain
        bare.explain_revoke(*ITEM)
    assert ei.value.code == aclgpu.ERR_FAILED_PRECONDITION and "no schema loaded" in ei.value.message
    with pytest.raises(aclgpu.AclError) as ei:
        bare.explain_ids(np.zeros(1, dtype=aclgpu.ITEM_DTYPE))
    want = ei.value.code
    with pytest.raises(aclgpu.AclError) as ei:  # the bulk form: whatever acl_explain_bulk_ids answers there
        bare.explain_revoke_ids(np.zeros(1, dtype=aclgpu.ITEM_DTYPE))
    assert ei.value.code == want


# ---------------------------------------------------------------- ABI
def test_prototypes_match_the_header(aclgpu, aclgpu_lib):
    text = open(HEADER).read()
    assert re.search(r"#define\s+ACL_EXPLAIN_REVOKE\s+16u", text) and aclgpu.EXPLAIN_REVOKE == 16
    hdr = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    hop, opts, item = C.POINTER(C.POINTER(aclgpu._lib.ExplainHop)), C.POINTER(aclgpu._lib.CallOpts), C.POINTER(aclgpu._lib.CheckItem)
    want = {
        "acl_explain_revoke_bulk_ids": [("acl_engine_t *", C.c_void_p), ("const acl_item_t *", C.c_void_p), ("size_t", C.c_size_t), ("uint8_t *", C.c_void_p),
                                        ("int32_t *", C.c_void_p), ("uint8_t *", C.c_void_p), ("uint32_t *", C.c_void_p), ("acl_explain_hop_t **", hop),
                                        ("const acl_call_opts_t *", opts)],
        "acl_explain_revoke": [("acl_engine_t *", C.c_void_p), ("const acl_check_item_t *", item), ("uint8_t *", C.POINTER(C.c_uint8)), ("int32_t *", C.POINTER(C.c_int32)),
                               ("uint32_t *", C.POINTER(C.c_uint32)), ("char **", C.POINTER(C.c_void_p)), ("const acl_call_opts_t *", opts)],
    }
    for name, params in want.items():
        assert name in aclgpu._lib.SYMBOLS and hasattr(aclgpu_lib, name)
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, name
        declared = [re.sub(r"\s+", " ", re.sub(r"\w+$", "", p.strip())).strip() for p in m.group(1).split(",")]
        assert declared == [t for t, _c in params], (name, declared)
        assert list(getattr(aclgpu_lib, name).argtypes) == [c for _t, c in params], name
    # the two forms take what their denial counterparts take, the records apart
    assert list(aclgpu_lib.acl_explain_revoke.argtypes) == list(aclgpu_lib.acl_explain_denial.argtypes)
    assert list(aclgpu_lib.acl_explain_revoke_bulk_ids.argtypes)[:7] == list(aclgpu_lib.acl_explain_denial_bulk_ids.argtypes)[:7]
    assert aclgpu.HOP_DTYPE.itemsize == C.sizeof(aclgpu._lib.ExplainHop) == 20

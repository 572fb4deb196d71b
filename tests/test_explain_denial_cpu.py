"""Explain for denials without a GPU: the ABI of acl_explain_denial*, the refusals of a store-only engine, and the host half (acl_selfcheck_denial_grants:
states -> grants, a pure function of the schema) held to tests/denial_checker.py's closures on hand schemas and to both oracles on random graphs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import denial_checker as D

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aclgpu.h")


@pytest.fixture(scope="module")
def aclgpu(aclgpu_lib):
    import aclgpu as m
    return m


def store(aclgpu, schema, rels=()):
    e = aclgpu.Engine(schema, store_only=True)
    items = list(D.as_dict(rels).items())
    for b in range(0, len(items), 1000):
        e.write([(aclgpu.OP_TOUCH, r, exp) for r, exp in items[b:b + 1000]])
    return e


def host_grants(e, schema, rels, root, stype, srel="", refs=False, states=None, now=0):
    """grants of the selfcheck, by name, for the states of root's closure (or the given {state: level})"""
    defs = D.parse_schema(schema)
    clos = D.closure(defs, rels, root, now, refs=refs) if states is None else states
    for (t, o, _m) in clos:
        e.intern(t, o)
    recs = e.selfcheck_denial_grants(root[0], root[2], stype, srel, D.encode_states(e, D.slot_table(e, schema), clos))
    return D.name_grants(e, schema, recs)


def expected(schema, rels, root, stype, srel="", now=0):
    defs = D.parse_schema(schema)
    return {k + (lv,) for k, lv in D.grants_of(defs, D.closure(defs, rels, root, now), stype, srel).items()}


# ---------------------------------------------------------------- ABI
def test_header_binding_and_struct_agree(aclgpu, aclgpu_lib, tmp_path):
    for name in ("acl_explain_denial_bulk_ids", "acl_explain_denial", "acl_selfcheck_denial_grants"):
        assert name in aclgpu._lib.SYMBOLS and hasattr(aclgpu_lib, name)
    ct = aclgpu._lib.Grant
    src = tmp_path / "grant.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "aclgpu.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %u\\n", sizeof(acl_grant_t), '
                   'offsetof(acl_grant_t, rtype), offsetof(acl_grant_t, relation), offsetof(acl_grant_t, rid), offsetof(acl_grant_t, level), ACL_EXPLAIN_DENIAL); return 0; }\n')
    exe = tmp_path / "grant"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert out == [12, 0, 2, 4, 8, aclgpu.EXPLAIN_DENIAL] == [C.sizeof(ct)] + [getattr(ct, f).offset for f, _t in ct._fields_] + [8]
    assert aclgpu.GRANT_DTYPE.itemsize == 12 and [aclgpu.GRANT_DTYPE.fields[f][1] for f, _t in ct._fields_] == out[1:5]


def test_store_only_engine_refuses(aclgpu):
    e = store(aclgpu, D.GROUPS, [("doc", "d", "viewer", "user", "u", "")])
    with pytest.raises(aclgpu.AclError) as ei:
        e.explain_denial_ids(e.make_items("doc", "view", [0], "user", "", [0]))
    assert ei.value.code == aclgpu.ERR_UNAVAILABLE
    with pytest.raises(aclgpu.AclError) as ei:
        e.explain_denial("doc", "d", "view", "user", "bob")
    assert ei.value.code == aclgpu.ERR_UNAVAILABLE
    with pytest.raises(aclgpu.AclError) as ei:  # the API's validation comes first, as for lookup_subjects
        e.explain_denial("doc", "d", "view", "user", "b*b")
    assert ei.value.code == aclgpu.ERR_INVALID_ARGUMENT


# ---------------------------------------------------------------- the host half on hand schemas
CHAIN = "definition user {}\ndefinition doc {\n relation r: user\n permission c = r\n permission b = c\n permission a = b\n}"
CYCLE = "definition user {}\ndefinition doc {\n relation r1: user\n relation r2: user\n permission p = q + r1\n permission q = p + r2\n}"
ARROW = """definition user {}
definition namespace {
  relation editor: user
  permission edit = editor
}
definition doc {
  relation namespace: namespace
  relation viewer: user
  relation editor: user
  permission edit = editor + namespace->edit
  permission view = viewer + edit
}"""
WILD = "definition user {}\ndefinition doc {\n relation open: user | user:*\n relation anyone: user:*\n relation team: user\n permission view = open + anyone + team\n}"
USERSET = """definition user {}
definition group {
  relation member: user | group#member
}
definition doc {
  relation viewer: user | group#member
  relation auditor: group#member
  permission view = viewer + auditor
}"""


def test_reference_chain(aclgpu):
    e = store(aclgpu, CHAIN)
    assert host_grants(e, CHAIN, {}, ("doc", "d", "a"), "user") == [("doc", "d", "r", 4)]
    assert host_grants(e, CHAIN, {}, ("doc", "d", "a"), "user", refs=True) == [("doc", "d", "r", 4)]
    assert set(host_grants(e, CHAIN, {}, ("doc", "d", "a"), "user")) == expected(CHAIN, {}, ("doc", "d", "a"), "user")


def test_reference_cycle_ends(aclgpu):
    e = store(aclgpu, CYCLE)
    got = host_grants(e, CYCLE, {}, ("doc", "d", "p"), "user")
    assert got == [("doc", "d", "r1", 2), ("doc", "d", "r2", 3)]
    assert set(got) == expected(CYCLE, {}, ("doc", "d", "p"), "user")


def test_arrows_are_the_devices_not_the_hosts(aclgpu):
    rels = {("doc", "d", "namespace", "namespace", "n", ""): 0}
    e = store(aclgpu, ARROW, rels)
    root = ("doc", "d", "view")
    alone = host_grants(e, ARROW, rels, root, "user", states={root: 1})
    assert alone == [("doc", "d", "viewer", 2), ("doc", "d", "editor", 3)]  # the namespace is a state the walk returns, not one the host derives
    full = host_grants(e, ARROW, rels, root, "user")
    assert full == alone + [("namespace", "n", "editor", 4)]  # view 1, edit 2, n#edit 3, n#editor 4
    assert set(full) == expected(ARROW, rels, root, "user")


def test_wildcard_forms(aclgpu):
    e = store(aclgpu, WILD)
    got = host_grants(e, WILD, {}, ("doc", "d", "view"), "user")
    assert got == [("doc", "d", "open", 2), ("doc", "d", "team", 2)]  # `anyone` takes user:* only: no grant for a named user
    assert set(got) == expected(WILD, {}, ("doc", "d", "view"), "user")


def test_userset_subject_class(aclgpu):
    rels = {("doc", "d", "viewer", "group", "g", "member"): 0, ("group", "g", "member", "group", "h", "member"): 0}
    e = store(aclgpu, USERSET, rels)
    root = ("doc", "d", "view")
    got = host_grants(e, USERSET, rels, root, "group", "member")
    assert got == [("doc", "d", "viewer", 2), ("doc", "d", "auditor", 2), ("group", "g", "member", 3), ("group", "h", "member", 4)]
    assert set(got) == expected(USERSET, rels, root, "group", "member")
    users = host_grants(e, USERSET, rels, root, "user")  # `auditor` holds no relationship anywhere and takes no user; `viewer` and the groups do
    assert users == [("doc", "d", "viewer", 2), ("group", "g", "member", 3), ("group", "h", "member", 4)]


def test_relation_without_relationships_is_a_grant(aclgpu):
    e = store(aclgpu, USERSET)
    assert host_grants(e, USERSET, {}, ("doc", "nobody-wrote-me", "view"), "group", "member") == [("doc", "nobody-wrote-me", "viewer", 2), ("doc", "nobody-wrote-me", "auditor", 2)]


def test_levels_beyond_fifty_are_dropped(aclgpu):
    e = store(aclgpu, CHAIN)
    at = lambda m, lv: host_grants(e, CHAIN, {}, ("doc", "d", "a"), "user", states={("doc", "d", m): lv})
    assert at("r", 50) == [("doc", "d", "r", 50)]
    assert at("c", 49) == [("doc", "d", "r", 50)]
    assert at("c", 50) == [] and at("a", 48) == []  # the reference would land at 51
    both = host_grants(e, CHAIN, {}, ("doc", "d", "a"), "user", states={("doc", "d", "a"): 40, ("doc", "d", "c"): 7, ("doc", "d", "r"): 9})
    assert both == [("doc", "d", "r", 8)]  # once, at its least level


def test_a_wide_permission_pushes_its_last_reference(aclgpu):
    """the schema the GPU file uses for a non-inlined computed userset does hold an OP_PUSH_SAME op, and the host half derives the same grants either way"""
    rels = {("doc", "d", "viewer", "group", "g", "member"): 0}
    e = store(aclgpu, D.PUSHED, rels)
    ops = e.selfcheck_explain_ops()
    slots = D.slot_table(e, D.PUSHED)
    assert any(int(o["kind"]) & 8 and int(o["slot"]) == slots[("doc", "big")] for o in ops)  # (csrc/plan.hpp OP_PUSH_SAME)
    want = [("doc", "d", f"r{i}", 2) for i in range(D.PUSHED_RELATIONS)] + [("doc", "d", "viewer", 3), ("group", "g", "member", 4)]
    for refs in (False, True):
        assert host_grants(e, D.PUSHED, rels, ("doc", "d", "big"), "user", refs=refs) == want


def test_selfcheck_refuses_bad_states(aclgpu):
    e = store(aclgpu, CHAIN)
    for bad in ([(0, 99 | (1 << 16))], [(0, 1)], [(0, 1 | (51 << 16))]):
        with pytest.raises(aclgpu.AclError) as ei:
            e.selfcheck_denial_grants("doc", "a", "user", "", bad)
        assert ei.value.code == aclgpu.ERR_INVALID_ARGUMENT


# ---------------------------------------------------------------- random graphs: the host half held to both oracles
@pytest.mark.parametrize("seed", D.SEEDS)
@pytest.mark.parametrize("family", sorted(D.FAMILIES))
def test_random_graphs_host_half(aclgpu, family, seed):
    schema, rels, items = D.random_graph(family, seed)
    orcs = D.Oracles(schema, rels)
    denied = D.denied_items(orcs, items)
    e = store(aclgpu, schema, rels)
    for k, it in enumerate(denied):
        got = host_grants(e, schema, rels, it[:3], it[3], it[5], refs=bool(k & 1))
        D.check_grants(orcs, it, got, seed=seed)

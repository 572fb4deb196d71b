"""Explain for denials on the GPU (k_reach_local + engine_denial.cpp) through the C ABI's Python mirror.

acl_explain_denial*(item) = Check(item) + for every item denied without error on a monotone permission ALL single relationships `o#r@subject` whose write
would grant it, each with the dispatch level at which a Check finds it.  Every answer goes through ONE checker (tests/denial_checker.py check_grants), which
holds it to both oracles: each listed relationship, written alone, makes both answer HAS at exactly that level; every other relationship with that subject that
the schema allows does not."""
import ctypes
import random

import numpy as np
import pytest

from oracle.pyoracle import parse_schema
from tests import denial_checker as D

pytestmark = pytest.mark.gpu

PERM_NO, PERM_HAS = 1, 2


@pytest.fixture(scope="module")
def aclgpu(aclgpu_lib):
    import aclgpu as m
    return m


@pytest.fixture(scope="module")
def C4(aclgpu):
    from aclgpu import workloads
    return workloads.SCHEMA_C4


def engine(aclgpu, schema, rels=(), now=None):
    e = aclgpu.Engine(schema, device=0)
    if now is not None:
        e.set_now(now)
    items = list(D.as_dict(rels).items())
    for b in range(0, len(items), 1000):
        e.write([(aclgpu.OP_TOUCH, r, exp) for r, exp in items[b:b + 1000]])
    return e


def ids_of(e, items):
    """named items as acl_item_t records; a name the engine does not know gets an id beyond its type's objects (resource: count + 5, subject: count + 7)"""
    out = []
    for (rt, rid, perm, st, sid, srel) in items:
        r, s = e.find(rt, rid), e.find(st, sid)
        out.append(e.make_items(rt, perm, [e.object_count(rt) + 5 if r is None else r], st, srel, [e.object_count(st) + 7 if s is None else s]))
    return np.concatenate(out)


def named(e, schema, item, recs):
    """acl_grant_t records of `item` -> [(rtype, rid, relation, level)] in the records' order, which is asserted to be the contract's"""
    defs = parse_schema(schema)
    tname = {e.type_id(t): t for t in defs}
    keys = [(int(g["level"]), int(g["rtype"]), int(g["relation"]), int(g["rid"])) for g in recs]
    assert keys == sorted(keys) and len(set(k[1:] for k in keys)) == len(keys)
    out = []
    for g in recs:
        t = tname[int(g["rtype"])]
        name = e.object_name(t, int(g["rid"]))
        if name is None:  # only the item's own resource may be an object without a name
            assert t == item[0] and e.find(t, item[1]) is None and int(g["rid"]) == e.object_count(t) + 5
            name = item[1]
        out.append((t, name, list(defs[t].members)[int(g["relation"])], int(g["level"])))
    return out


def ask(aclgpu, e, schema, items):
    """the named items in ONE call of the ids form and one call each of the string form: the two agree with each other and with Check.
    -> [(perm, err, flags, [(rtype, rid, relation, level)])]"""
    from aclgpu.text import parse_relationship
    ids = ids_of(e, items)
    perm, err, flags, off, recs = e.explain_denial_ids(ids)
    cperm, cerr = e.check_bulk_ids(ids)
    assert np.array_equal(perm, cperm) and np.array_equal(err, cerr)
    assert off[0] == 0 and off[-1] == recs.size and np.all(np.diff(off.astype(np.int64)) >= 0)
    out = []
    for i, it in enumerate(items):
        grants = named(e, schema, it, recs[off[i]:off[i + 1]])
        p, er, fl, lines = e.explain_denial(*it)
        assert (p, er, fl) == (int(perm[i]), int(err[i]), int(flags[i])) and (p, er) == e.check(*it)
        assert [parse_relationship(ln) for ln in lines] == [(t, o, r, it[3], it[4], it[5]) for (t, o, r, _lv) in grants]
        if not fl & aclgpu.EXPLAIN_DENIAL:
            assert grants == []
        else:
            assert (p, er) == (PERM_NO, 0)
        out.append((p, er, fl, grants))
    return out


def explained(aclgpu, e, orcs, item, others=True):
    """one denied item: asked both ways, held to the oracles; -> its grants"""
    (p, er, fl, grants), = ask(aclgpu, e, orcs.schema, [item])
    assert (p, er, fl) == (PERM_NO, 0, aclgpu.EXPLAIN_DENIAL), (item, p, er, fl)
    D.check_grants(orcs, item, grants, others=others)
    return grants


# ---------------------------------------------------------------- 1. hand graphs
def test_direct_relation(aclgpu, C4):
    rels = [("pod", "p", "viewer", "user", "alice", "")]
    with engine(aclgpu, C4, rels) as e:
        assert explained(aclgpu, e, D.Oracles(C4, rels), ("pod", "p", "viewer", "user", "bob", "")) == [("pod", "p", "viewer", 1)]
        assert explained(aclgpu, e, D.Oracles(C4, rels), ("pod", "p", "creator", "user", "alice", "")) == [("pod", "p", "creator", 1)]
        assert explained(aclgpu, e, D.Oracles(C4, rels), ("pod", "p", "namespace", "user", "alice", "")) == []  # `namespace` takes no user: nothing to write


def test_union_with_an_arrow(aclgpu, C4):
    rels = [("pod", "p", "namespace", "namespace", "n", ""), ("pod", "p", "creator", "user", "alice", ""), ("namespace", "n", "viewer", "user", "carol", "")]
    with engine(aclgpu, C4, rels) as e:
        got = explained(aclgpu, e, D.Oracles(C4, rels), ("pod", "p", "view", "user", "bob", ""))
        assert got == [("pod", "p", "viewer", 2), ("pod", "p", "creator", 2), ("namespace", "n", "viewer", 3), ("namespace", "n", "creator", 3)]


def test_nested_groups_three_deep(aclgpu, C4):
    rels = [("pod", "p", "viewer", "group", "a", "member"), ("group", "a", "member", "group", "b", "member"), ("group", "b", "member", "group", "c", "member"),
            ("group", "c", "member", "user", "alice", "")]
    with engine(aclgpu, C4, rels) as e:
        got = explained(aclgpu, e, D.Oracles(C4, rels), ("pod", "p", "view", "user", "bob", ""))
        assert got == [("pod", "p", "viewer", 2), ("pod", "p", "creator", 2), ("group", "a", "member", 3), ("group", "b", "member", 4), ("group", "c", "member", 5)]


def test_diamond_is_reported_once_at_its_least_level(aclgpu, C4):
    rels = [("pod", "p", "viewer", "group", "d", "member"), ("pod", "p", "viewer", "group", "a", "member"), ("group", "a", "member", "group", "b", "member"),
            ("group", "b", "member", "group", "d", "member")]  # d at level 3 directly, and at 5 through a and b
    with engine(aclgpu, C4, rels) as e:
        got = explained(aclgpu, e, D.Oracles(C4, rels), ("pod", "p", "view", "user", "bob", ""))
        # (the order among equals of one level follows the objects' ids, which `named` has checked)
        assert sorted(got) == sorted([("pod", "p", "viewer", 2), ("pod", "p", "creator", 2), ("group", "a", "member", 3), ("group", "d", "member", 3), ("group", "b", "member", 4)])
    rels = [("pod", "p", "viewer", "group", "d", "member"), ("pod", "p", "namespace", "namespace", "n", ""), ("namespace", "n", "viewer", "group", "d", "member")]
    with engine(aclgpu, C4, rels) as e:  # d at 3 through the pod's viewers, and at 4 through the namespace's
        got = explained(aclgpu, e, D.Oracles(C4, rels), ("pod", "p", "view", "user", "bob", ""))
        assert got.count(("group", "d", "member", 3)) == 1 and [g for g in got if g[1] == "d"] == [("group", "d", "member", 3)]


def test_cycle_of_two_groups(aclgpu, C4):
    # Both oracles follow the cycle down to the depth limit, so a Check that meets it and finds nothing answers ERR: the item's own error, flag 0, no grants
    # (what such a Check has looked at is not known to be complete).  The oracles decide which of the two this test asserts.
    rels = [("pod", "p", "viewer", "group", "a", "member"), ("group", "a", "member", "group", "b", "member"), ("group", "b", "member", "group", "a", "member")]
    orcs = D.Oracles(C4, rels)
    item = ("pod", "p", "view", "user", "bob", "")
    with engine(aclgpu, C4, rels) as e:
        if orcs.denied(item):
            assert sorted(explained(aclgpu, e, orcs, item)) == sorted([("pod", "p", "viewer", 2), ("pod", "p", "creator", 2), ("group", "a", "member", 3), ("group", "b", "member", 4)])
        else:
            (_p, cerr), y = orcs.check(item)
            assert cerr == D.orc.ERR_DEPTH and y == "ERR"
            (p, er, fl, grants), = ask(aclgpu, e, C4, [item])
            assert er == aclgpu.ERR_DEPTH and fl == 0 and grants == []
        # an item that never reaches the cycle is explained as ever
        assert explained(aclgpu, e, orcs, ("pod", "q", "view", "user", "bob", "")) == [("pod", "q", "viewer", 2), ("pod", "q", "creator", 2)]


COMPUTED = """
definition user {}
definition group {
  relation member: user | group#member
}
definition doc {
  relation owner: user
  relation editor: user | group#member
  relation viewer: user | group#member
  relation banned: user
  permission edit = editor + owner
  permission view = viewer + edit
  permission safe = viewer - banned
  permission audit = view + safe
}
"""


def test_computed_usersets_inlined_and_pushed(aclgpu):
    rels = [("doc", "d", "editor", "group", "g", "member"), ("group", "g", "member", "user", "alice", "")]
    with engine(aclgpu, COMPUTED, rels) as e:  # view -> edit is inlined into view's program
        got = explained(aclgpu, e, D.Oracles(COMPUTED, rels), ("doc", "d", "view", "user", "bob", ""))
        assert got == [("doc", "d", "viewer", 2), ("doc", "d", "owner", 3), ("doc", "d", "editor", 3), ("group", "g", "member", 4)]
    # a permission of more operands than a program inlines: `tail` is a state of its own on the same object (OP_PUSH_SAME; the CPU file checks that it is)
    rels = [("doc", "d", "viewer", "group", "g", "member"), ("doc", "d", "r7", "user", "alice", "")]
    with engine(aclgpu, D.PUSHED, rels) as e:
        got = explained(aclgpu, e, D.Oracles(D.PUSHED, rels), ("doc", "d", "big", "user", "bob", ""))
        assert got == [("doc", "d", f"r{i}", 2) for i in range(D.PUSHED_RELATIONS)] + [("doc", "d", "viewer", 3), ("group", "g", "member", 4)]


def test_subject_with_a_relation(aclgpu, C4):
    rels = [("pod", "p", "viewer", "group", "a", "member"), ("group", "a", "member", "group", "b", "member"), ("pod", "p", "namespace", "namespace", "n", "")]
    with engine(aclgpu, C4, rels) as e:
        got = explained(aclgpu, e, D.Oracles(C4, rels), ("pod", "p", "view", "group", "x", "member"))
        assert got == [("pod", "p", "viewer", 2), ("group", "a", "member", 3), ("namespace", "n", "viewer", 3), ("group", "b", "member", 4)]
        (p, er, fl, grants), = ask(aclgpu, e, C4, [("pod", "p", "view", "group", "b", "member")])  # reached: granted, Explain's business
        assert (p, er, fl, grants) == (PERM_HAS, 0, 0, [])


WILD = """
definition user {}
definition pod {
  relation open: user | user:*
  relation anyone: user:*
  relation team: user
  permission view = open + anyone + team
}
"""


def test_wildcards(aclgpu):
    rels = [("pod", "other", "open", "user", "*", ""), ("pod", "other", "anyone", "user", "*", ""), ("pod", "p", "team", "user", "alice", "")]
    with engine(aclgpu, WILD, rels) as e:  # a wildcard relationship on another pod changes nothing; `anyone` takes user:* only and is no grant
        assert explained(aclgpu, e, D.Oracles(WILD, rels), ("pod", "p", "view", "user", "bob", "")) == [("pod", "p", "open", 2), ("pod", "p", "team", 2)]
        (p, er, fl, grants), = ask(aclgpu, e, WILD, [("pod", "other", "view", "user", "bob", "")])
        assert (p, er, fl, grants) == (PERM_HAS, 0, 0, [])


EXPIRING = """
definition user {}
definition group {
  relation member: user with expiration | group#member with expiration
}
definition pod {
  relation viewer: user with expiration | group#member
  permission view = viewer
}
"""


def test_expired_relationships(aclgpu):
    rels = {("pod", "p", "viewer", "user", "bob", ""): 500, ("pod", "p", "viewer", "group", "g", "member"): 0, ("group", "g", "member", "group", "old", "member"): 500,
            ("group", "g", "member", "group", "live", "member"): 5000}
    with engine(aclgpu, EXPIRING, rels, now=1000) as e:  # bob's own grant has run out: it is listed again; the group behind an expired hop is not reached
        got = explained(aclgpu, e, D.Oracles(EXPIRING, rels, now=1000), ("pod", "p", "view", "user", "bob", ""))
        assert got == [("pod", "p", "viewer", 2), ("group", "g", "member", 3), ("group", "live", "member", 4)]


# ---------------------------------------------------------------- 2. unknown resources and odd names
def test_unknown_names(aclgpu, C4):
    rels = [("pod", "ns/a|b=c+d", "viewer", "group", "g/1|2", "member"), ("group", "g/1|2", "member", "user", "al=ice+x", "")]
    orcs = D.Oracles(C4, rels)
    with engine(aclgpu, C4, rels) as e:
        ghost = explained(aclgpu, e, orcs, ("pod", "nobody-wrote-me", "view", "user", "al=ice+x", ""))
        assert ghost == [("pod", "nobody-wrote-me", "viewer", 2), ("pod", "nobody-wrote-me", "creator", 2)]
        known = explained(aclgpu, e, orcs, ("pod", "ns/a|b=c+d", "view", "user", "bob/x|y=z+w", ""))  # a subject nobody has written
        assert known == [("pod", "ns/a|b=c+d", "viewer", 2), ("pod", "ns/a|b=c+d", "creator", 2), ("group", "g/1|2", "member", 3)]
        e.touch(("namespace", "n", "creator", "user", "carol", ""))
        orcs.touch_all([("namespace", "n", "creator", "user", "carol", "")])
        assert explained(aclgpu, e, orcs, ("pod", "ns/a|b=c+d", "view", "user", "carol", "")) == known  # the same grants as any other subject of the class
        assert e.explain_denial("pod", "nobody-wrote-me", "view", "user", "bob")[3] == ["pod:nobody-wrote-me#viewer@user:bob", "pod:nobody-wrote-me#creator@user:bob"]


# ---------------------------------------------------------------- 3. flags
BAN = """
definition user {}
definition group {
  relation member: user
}
definition doc {
  relation viewer: user
  relation banned: user
  relation editor: user | group#member
  permission view = viewer - banned
  permission edit = editor
}
"""


def test_flags_in_a_mixed_batch(aclgpu, aclgpu_lib):
    rels = [("doc", "d", "viewer", "user", "a", ""), ("doc", "d", "viewer", "user", "b", ""), ("doc", "d", "banned", "user", "b", ""), ("doc", "d", "editor", "user", "a", ""),
            ("doc", "d", "editor", "group", "g", "member")]
    items = [("doc", "d", "edit", "user", "a", ""),            # granted: 0
             ("doc", "d", "edit", "user", "b", ""),            # denied on a monotone permission: explained
             ("doc", "d", "view", "user", "b", ""),            # a NO on `viewer - banned`: unsupported
             ("doc", "d", "view", "user", "a", ""),            # granted (non-monotone): 0
             ("group", "g", "member", "user", "b", ""),        # another resource type and permission
             ("doc", "d", "edit", "group", "h", "member")]     # another subject class
    orcs = D.Oracles(BAN, rels)
    with engine(aclgpu, BAN, rels) as e:
        got = ask(aclgpu, e, BAN, items)
        assert [(p, er, fl) for (p, er, fl, _g) in got] == [(PERM_HAS, 0, 0), (PERM_NO, 0, aclgpu.EXPLAIN_DENIAL), (PERM_NO, 0, aclgpu.EXPLAIN_UNSUPPORTED), (PERM_HAS, 0, 0),
                                                             (PERM_NO, 0, aclgpu.EXPLAIN_DENIAL), (PERM_NO, 0, aclgpu.EXPLAIN_DENIAL)]
        assert got[1][3] == [("doc", "d", "editor", 2), ("group", "g", "member", 3)] and got[4][3] == [("group", "g", "member", 1)] and got[5][3] == [("doc", "d", "editor", 2)]
        for i in (1, 4, 5):
            D.check_grants(orcs, items[i], got[i][3])
        # an unknown permission is the item's own error: flag 0, nothing else
        p, er, fl, lines = e.explain_denial("doc", "d", "nosuchperm", "user", "a")
        assert (p, er) == e.check("doc", "d", "nosuchperm", "user", "a") and er != 0 and fl == 0 and lines == []
        bad = ids_of(e, items[1:2])
        bad["permission"] = 77
        perm, err, flags, off, recs = e.explain_denial_ids(bad)
        cperm, cerr = e.check_bulk_ids(bad)
        assert int(err[0]) == int(cerr[0]) != 0 and int(perm[0]) == int(cperm[0]) and int(flags[0]) == 0 and recs.size == 0
        # Explain itself still answers a denied item with flag 0 and nothing else
        for it in items[1:3]:
            assert e.explain(*it) == (PERM_NO, 0, 0, [])
        # n == 0
        perm, err, flags, off, recs = e.explain_denial_ids(np.zeros(0, dtype=aclgpu.ITEM_DTYPE))
        assert perm.size == err.size == flags.size == recs.size == 0 and off.tolist() == [0]
        # acl_call_opts_t: already cancelled / already past its deadline are refused; the same call afterwards returns the same bytes
        ids = ids_of(e, items)
        first = e.explain_denial_ids(ids)
        flag = ctypes.c_int32(1)
        with pytest.raises(aclgpu.AclError) as x:
            e.explain_denial_ids(ids, cancel=flag)
        assert x.value.code == aclgpu.ERR_CANCELLED
        with pytest.raises(aclgpu.AclError) as x:
            e.explain_denial_ids(ids, timeout_s=1e-9)
        assert x.value.code == aclgpu.ERR_DEADLINE_EXCEEDED
        flag.value = 0
        again = e.explain_denial_ids(ids, cancel=flag, timeout_s=60.0)
        assert all(u.tobytes() == v.tobytes() for u, v in zip(again, first))
        # one shard of a sharded graph does not explain
        e._check(aclgpu_lib.acl_shard_configure(e._h, 0, 2))
        with pytest.raises(aclgpu.AclError) as x:
            e.explain_denial_ids(ids)
        assert x.value.code == aclgpu.ERR_FAILED_PRECONDITION
        with pytest.raises(aclgpu.AclError) as x:
            e.explain_denial(*items[1])
        assert x.value.code == aclgpu.ERR_FAILED_PRECONDITION


# ---------------------------------------------------------------- 4. sharing: many items about one resource cost one walk
def test_three_hundred_items_about_one_resource(aclgpu, C4):
    rels = [("pod", "p", "viewer", "group", "a", "member"), ("group", "a", "member", "group", "b", "member"), ("pod", "p", "namespace", "namespace", "n", "")]
    rels += [("group", "z", "member", "user", f"u{i}", "") for i in range(150)] + [("group", f"h{i}", "member", "user", "u0", "") for i in range(150)]
    orcs = D.Oracles(C4, rels)
    items = [("pod", "p", "view", "user", f"u{i}", "") for i in range(150)] + [("pod", "p", "view", "group", f"h{i}", "member") for i in range(150)]
    with engine(aclgpu, C4, rels) as e:
        ids = ids_of(e, items)
        perm, err, flags, off, recs = e.explain_denial_ids(ids)
        assert np.all(perm == PERM_NO) and not err.any() and np.all(flags == aclgpu.EXPLAIN_DENIAL)
        per = [named(e, C4, it, recs[off[i]:off[i + 1]]) for i, it in enumerate(items)]
        users = [("pod", "p", "viewer", 2), ("pod", "p", "creator", 2), ("group", "a", "member", 3), ("namespace", "n", "viewer", 3), ("namespace", "n", "creator", 3),
                 ("group", "b", "member", 4)]
        groups = [g for g in users if g[2] != "creator"]
        assert all(p == users for p in per[:150]) and all(p == groups for p in per[150:])  # per class, identical within a class
        D.check_grants(orcs, items[3], per[3])
        D.check_grants(orcs, items[200], per[200])
        again = e.explain_denial_ids(ids)
        assert all(u.tobytes() == v.tobytes() for u, v in zip(again, (perm, err, flags, off, recs)))


# ---------------------------------------------------------------- 5. the depth limit
def chain(n):
    return [("pod", "p", "viewer", "group", "g0", "member")] + [("group", f"g{i}", "member", "group", f"g{i + 1}", "member") for i in range(n)]


def test_depth_limit(aclgpu, C4):
    item = ("pod", "p", "view", "user", "bob", "")
    n = 40  # lengthened on the oracles until both answer ERR: n is then the first chain that is too long
    while True:
        orcs = D.Oracles(C4, chain(n))
        (p, er), y = orcs.check(item)
        if y == "ERR":
            assert er == D.orc.ERR_DEPTH
            break
        assert (p, er, y) == (D.ORC_NO, 0, "NO") and n < 60
        n += 1
    rels = chain(n - 1)  # the longest chain that is still NO without error
    with engine(aclgpu, C4, rels) as e:
        got = explained(aclgpu, e, D.Oracles(C4, rels), item)
        assert got == [("pod", "p", "viewer", 2), ("pod", "p", "creator", 2)] + [("group", f"g{i}", "member", 3 + i) for i in range(n)]
        assert got[-1][3] == 50
    with engine(aclgpu, C4, chain(n)) as e:  # one more group: the item's own error, flag 0, no grants
        (p, er, fl, grants), = ask(aclgpu, e, C4, [item])
        assert er == aclgpu.ERR_DEPTH and fl == 0 and grants == []


# ---------------------------------------------------------------- 6. shapes where the kernel can go wrong
def by_ids(e, schema, recs):
    """acl_grant_t records of objects loaded by id -> {(rtype, str(id), relation): level}"""
    defs = parse_schema(schema)
    tname = {e.type_id(t): t for t in defs}
    return {(tname[int(g["rtype"])], str(int(g["rid"])), list(defs[tname[int(g["rtype"])]].members)[int(g["relation"])]): int(g["level"]) for g in recs}


def star(n_groups, second=0):
    """pods 0 and 1 -> group 0 -> groups 1..n_groups (one userset row), the first `second` of which hold one more group each; objects named by their ids"""
    rels = [("pod", "0", "viewer", "group", "0", "member"), ("pod", "1", "viewer", "group", "0", "member")]
    rels += [("group", "0", "member", "group", str(i), "member") for i in range(1, n_groups + 1)]
    rels += [("group", str(i), "member", "group", str(n_groups + i), "member") for i in range(1, second + 1)]
    return rels


def load_by_ids(e, rels):
    by = {}
    for (rt, rid, rel, st, sid, sr) in rels:
        by.setdefault((rt, rel, st, sr), []).append((int(rid), int(sid)))
    for (rt, rel, st, sr), pairs in by.items():
        a = np.array(pairs, dtype=np.uint32)
        e.add_edges(rt, rel, st, sr, a[:, 0], a[:, 1])


def large_case(aclgpu, C4, rels, pods, subject=9):
    """denied pod#view items of user `subject` (an id no relationship names) on a graph loaded by id: the grant sets equal the checker's closures as sets with
    levels, and a seeded sample of 50 grants goes through check_grants.  -> the engine's overflow_retries the call moved"""
    orcs = D.Oracles(C4, rels)
    with aclgpu.Engine(C4, device=0) as e:
        load_by_ids(e, rels)
        items = e.make_items("pod", "view", pods, "user", "", [subject] * len(pods))
        for _ in range(3):  # (the snapshot and whatever the Check learns about this graph on its first calls are behind us)
            e.check_bulk_ids(items)
        s0 = e.stats()["overflow_retries"]
        e.check_bulk_ids(items)
        s1 = e.stats()["overflow_retries"]
        perm, err, flags, off, recs = e.explain_denial_ids(items)
        moved = (e.stats()["overflow_retries"] - s1) - (s1 - s0)  # (beyond what the Check inside the call accounts for)
        print(f"overflow_retries: a Check moves {s1 - s0}, the call moved {moved} more")
        assert np.all(perm == PERM_NO) and not err.any() and np.all(flags == aclgpu.EXPLAIN_DENIAL)
        for i, pod in enumerate(pods):
            got = by_ids(e, C4, recs[off[i]:off[i + 1]])
            assert len(got) == off[i + 1] - off[i]
            want = D.grants_of(orcs.defs, D.closure(orcs.defs, orcs.rels, ("pod", str(pod), "view")), "user")
            assert got == want, (pod, len(got), len(want))
        again = e.explain_denial_ids(items)
        assert all(u.tobytes() == v.tobytes() for u, v in zip(again, (perm, err, flags, off, recs)))
        sample = random.Random(5).sample(sorted(got.items()), min(50, len(got)))
        D.check_grants(orcs, ("pod", str(pods[-1]), "view", "user", str(subject), ""), [k + (lv,) for k, lv in sample], others=False)
        return moved


def test_a_row_that_spans_rounds_and_a_closure_of_several(aclgpu, C4):
    # one userset row of 2 500 groups (a task that spans three rounds of 1 024 children), 300 of them with a group of their own: 2 800 states at two levels,
    # which is more than one round of (state, op) pairs per level
    large_case(aclgpu, C4, star(2500, second=300), [0])


def test_log_and_region_redo(aclgpu, C4):
    # a closure of 17 000 states outgrows the first log of 16 384 entries: the chunk is walked again with a larger one ...
    rels = star(17000)
    moved = large_case(aclgpu, C4, rels, [0])
    assert moved >= 1
    # ... and two of them outgrow the first output region of 32 768 records: the pass is redone with a larger region as well
    moved = large_case(aclgpu, C4, rels, [0, 1])
    assert moved >= 2


def test_seventy_resources_in_one_call(aclgpu, C4):
    rels = []
    for i in range(70):
        rels += [("pod", str(i), "viewer", "group", str(i % 9), "member"), ("pod", str(i), "namespace", "namespace", str(i % 4), "")]
    rels += [("group", str(i), "member", "group", str(10 + i), "member") for i in range(9)] + [("namespace", str(i), "viewer", "group", str(20 + i), "member") for i in range(4)]
    large_case(aclgpu, C4, rels, list(range(70)), subject=99)


# ---------------------------------------------------------------- 7. the random graphs of the CPU file, end to end
@pytest.mark.parametrize("seed", D.SEEDS)
@pytest.mark.parametrize("family", sorted(D.FAMILIES))
def test_random_graphs(aclgpu, family, seed):
    schema, rels, items = D.random_graph(family, seed)
    orcs = D.Oracles(schema, rels)
    denied = D.denied_items(orcs, items)  # (the condition on the graph is established on the oracle side, before the engine is asked)
    with engine(aclgpu, schema, rels) as e:
        for it, (p, er, fl, grants) in zip(denied, ask(aclgpu, e, schema, denied)):
            assert (p, er, fl) == (PERM_NO, 0, aclgpu.EXPLAIN_DENIAL), it
            D.check_grants(orcs, it, grants, seed=seed)

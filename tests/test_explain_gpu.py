"""Explain on the GPU (k_explain_local + engine_explain.cpp) through the C ABI's Python mirror.

Explain(item) = Check(item) + a witness: perm / err are acl_check_bulk_ids' for the same items, and every item that a monotone permission grants comes with a
chain of stored relationships from its resource to its subject.  Every witness goes through ONE checker (tests/explain_checker.py): the hops are relationships
of the test's own set, they chain, and the hops alone -- loaded into an empty store under the same schema -- make both oracles' Check answer HAS."""
import ctypes

import numpy as np
import pytest

from oracle import orc
from oracle.pyoracle import ERR, HAS, NO, PyOracle, parse_schema
from tests import explain_checker as X

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


def namer(e, schema, named=True):
    """acl_explain_hop_t records -> (rtype, rid, rel, stype, sid, srel) tuples; named=False: objects loaded by id, spelled as their decimal ids"""
    defs = parse_schema(schema)
    tname = {e.type_id(t): t for t in defs}
    rname = {(e.type_id(t), e.relation_id(t, m)): m for t, d in defs.items() for m in d.members}
    obj = (lambda t, i: e.object_name(t, i)) if named else (lambda t, i: str(i))

    def conv(hops):
        out = []
        for h in hops:
            rt, st = tname[int(h["rtype"])], tname[int(h["stype"])]
            sid = "*" if int(h["flags"]) & 1 else obj(st, int(h["sid"]))
            srel = "" if int(h["srel"]) == 0xFFFF else rname[(int(h["stype"]), int(h["srel"]))]
            out.append((rt, obj(rt, int(h["rid"])), rname[(int(h["rtype"]), int(h["relation"]))], st, sid, srel))
        return out
    return conv


def item_ids(e, item):
    """a named item as one acl_item_t (every name known to the engine)"""
    rt, rid, perm, st, sid, srel = item
    return e.make_items(rt, perm, [e.find(rt, rid)], st, srel, [e.find(st, sid)])


def explain_both(aclgpu, e, schema, rels, item, exact=True):
    """Explain of one named item through BOTH entry points: they agree with each other and with Check, and the witness passes the checker.
    exact=False: the graph holds several chains of the least length -- either call may return any of them.  Returns (perm, err, flags, hops as tuples)."""
    from aclgpu.text import parse_relationship
    p, er, fl, lines = e.explain(*item)
    hops = [parse_relationship(ln) for ln in lines]
    assert (p, er) == e.check(*item)
    perm, err, flags, off, raw = e.explain_ids(item_ids(e, item))
    assert (int(perm[0]), int(err[0]), int(flags[0])) == (p, er, fl)
    assert off.tolist() == [0, len(raw)]
    ids_hops = namer(e, schema)(raw)
    assert len(ids_hops) == len(hops) and (ids_hops == hops or not exact)
    if fl & aclgpu.EXPLAIN_WITNESS:
        assert p == PERM_HAS and er == 0
        X.check_witness(schema, set(rels), item, hops)
        X.check_witness(schema, set(rels), item, ids_hops, replay_it=ids_hops != hops)
    else:
        assert hops == []
    return p, er, fl, hops


# ---------------------------------------------------------------- 1. small hand graphs, exact expectations
def test_direct_creator_is_one_hop(aclgpu, C4):
    rels = [("pod", "ns/a", "creator", "user", "u", ""), ("pod", "ns/a", "viewer", "user", "other", "")]
    with aclgpu.Engine(C4, device=0) as e:
        e.touch(*rels)
        p, er, fl, hops = explain_both(aclgpu, e, C4, rels, ("pod", "ns/a", "view", "user", "u", ""))
        assert (p, er, fl) == (PERM_HAS, 0, aclgpu.EXPLAIN_WITNESS) and hops == [rels[0]]


def test_namespace_arrow_through_nested_groups_is_the_four_hop_chain(aclgpu, C4):
    chain = [("pod", "ns/a", "namespace", "namespace", "ns", ""), ("namespace", "ns", "viewer", "group", "outer", "member"),
             ("group", "outer", "member", "group", "inner", "member"), ("group", "inner", "member", "user", "u", "")]
    rels = chain + [("pod", "ns/a", "viewer", "user", "other", ""), ("group", "outer", "member", "user", "other", ""), ("namespace", "ns", "creator", "user", "other", "")]
    with aclgpu.Engine(C4, device=0) as e:
        e.touch(*rels)
        p, er, fl, hops = explain_both(aclgpu, e, C4, rels, ("pod", "ns/a", "view", "user", "u", ""))
        assert (p, er, fl) == (PERM_HAS, 0, aclgpu.EXPLAIN_WITNESS) and hops == chain


def test_diamond_gives_the_short_chain(aclgpu, C4):
    short = [("pod", "p", "viewer", "group", "g1", "member"), ("group", "g1", "member", "user", "u", "")]
    rels = short + [("group", "g1", "member", "group", "g2", "member"), ("group", "g2", "member", "group", "g3", "member"),
                    ("group", "g3", "member", "group", "g4", "member"), ("group", "g4", "member", "user", "u", "")]
    with aclgpu.Engine(C4, device=0) as e:
        e.touch(*rels)
        _, _, fl, hops = explain_both(aclgpu, e, C4, rels, ("pod", "p", "view", "user", "u", ""))
        assert fl == aclgpu.EXPLAIN_WITNESS and hops == short


def test_subject_with_a_relation_ends_at_the_userset_hop(aclgpu, C4):
    rels = [("pod", "p", "viewer", "group", "g", "member"), ("group", "g", "member", "user", "u", ""), ("group", "g", "member", "group", "h", "member")]
    with aclgpu.Engine(C4, device=0) as e:
        e.touch(*rels)
        _, _, fl, hops = explain_both(aclgpu, e, C4, rels, ("pod", "p", "view", "group", "g", "member"))
        assert fl == aclgpu.EXPLAIN_WITNESS and hops == [rels[0]]
        _, _, fl, hops = explain_both(aclgpu, e, C4, rels, ("pod", "p", "view", "group", "h", "member"))
        assert fl == aclgpu.EXPLAIN_WITNESS and hops == [rels[0], rels[2]]
        # the reflexive item: granted by zero hops
        p, er, fl, hops = explain_both(aclgpu, e, C4, rels, ("group", "g", "member", "group", "g", "member"))
        assert (p, er, fl, hops) == (PERM_HAS, 0, aclgpu.EXPLAIN_WITNESS, [])


def test_no_and_unknown_names_are_answered_as_check_answers_them(aclgpu, C4):
    rels = [("pod", "p", "viewer", "user", "u", ""), ("pod", "q", "creator", "user", "v", "")]
    with aclgpu.Engine(C4, device=0) as e:
        e.touch(*rels)
        p, er, fl, hops = explain_both(aclgpu, e, C4, rels, ("pod", "q", "view", "user", "u", ""))
        assert (p, er, fl, hops) == (PERM_NO, 0, 0, [])
        for item in (("pod", "p", "view", "user", "nobody-wrote-this", ""), ("pod", "no-such-pod", "view", "user", "u", "")):
            p, er, fl, lines = e.explain(*item)
            assert (p, er) == e.check(*item) == (PERM_NO, 0) and fl == 0 and lines == []
        # an unknown permission is the item's own error, an ill-formed id fails the call: as acl_check_bulk
        p, er, fl, lines = e.explain("pod", "p", "nope", "user", "u")
        assert (p, er) == e.check("pod", "p", "nope", "user", "u") and er == aclgpu.ERR_FAILED_PRECONDITION and fl == 0 and lines == []
        with pytest.raises(aclgpu.AclError) as x:
            e.explain("pod", "not an id", "view", "user", "u")
        assert x.value.code == aclgpu.ERR_INVALID_ARGUMENT


def test_wildcard_hop_carries_the_flag(aclgpu):
    schema = """
definition user {}
definition group {
  relation member: user | group#member
}
definition doc {
  relation viewer: user | user:* | group#member
  permission view = viewer
}
"""
    rels = [("doc", "d", "viewer", "group", "g", "member"), ("doc", "open", "viewer", "user", "*", ""), ("group", "g", "member", "user", "u", "")]
    with aclgpu.Engine(schema, device=0) as e:
        e.touch(*rels)
        p, er, fl, hops = explain_both(aclgpu, e, schema, rels, ("doc", "open", "view", "user", "u", ""))
        assert (p, er, fl) == (PERM_HAS, 0, aclgpu.EXPLAIN_WITNESS) and hops == [rels[1]]
        _, _, _, _, raw = e.explain_ids(item_ids(e, ("doc", "open", "view", "user", "u", "")))
        assert int(raw[0]["flags"]) == aclgpu.HOP_WILDCARD and int(raw[0]["sid"]) == e.find("user", "*")
        _, _, _, hops = explain_both(aclgpu, e, schema, rels, ("doc", "d", "view", "user", "u", ""))
        assert hops == [rels[0], rels[2]]


# ---------------------------------------------------------------- 2. the depth limit
def depth_graph(n):
    return ([("pod", "p", "viewer", "group", "g0", "member")] + [("group", f"g{i}", "member", "group", f"g{i + 1}", "member") for i in range(n)] +
            [("group", f"g{n}", "member", "user", "u", "")])


def test_depth_limit_on_the_python_oracle(C4):
    for n, want in ((47, HAS), (48, ERR)):
        o = PyOracle(C4)
        for r in depth_graph(n):
            o.touch(*r)
        assert o.check("pod", "p", "view", "user", "u") == want


def test_depth_limit_witness_is_the_whole_chain(aclgpu, C4):
    item = ("pod", "p", "view", "user", "u", "")
    rels = depth_graph(47)
    assert len(rels) == 49
    with aclgpu.Engine(C4, device=0) as e:
        e.touch(*rels)
        p, er, fl, hops = explain_both(aclgpu, e, C4, rels, item)
        assert (p, er, fl) == (PERM_HAS, 0, aclgpu.EXPLAIN_WITNESS) and hops == rels
    rels = depth_graph(48)
    with aclgpu.Engine(C4, device=0) as e:
        e.touch(*rels)
        p, er, fl, hops = explain_both(aclgpu, e, C4, rels, item)
        assert er == aclgpu.ERR_DEPTH and (p, er) == e.check(*item) and fl == 0 and hops == []
        perm, err = e.check_bulk_ids(item_ids(e, item))
        assert int(err[0]) == aclgpu.ERR_DEPTH


# ---------------------------------------------------------------- 3. workload parity
@pytest.mark.parametrize("name", ["c3", "c4"])
def test_workload_parity(aclgpu, name):
    from aclgpu import workloads
    w = workloads.c3(scale=0.01) if name == "c3" else workloads.c4(scale=0.01, n_user=2000)
    n = 4096
    res, subj = w.res[:n], w.subj[:n]
    rt, pm, st = w.check
    edges = {}
    for ert, rel, est, srel, r, s in w.edges:
        edges.setdefault((ert, rel, est, srel), set()).update(((r.astype(np.uint64) << np.uint64(32)) | s.astype(np.uint64)).tolist())
    stored = lambda h: ((int(h[1]) << 32) | int(h[4])) in edges.get((h[0], h[2], h[3], h[5]), ())  # noqa: E731
    o = orc.Oracle(w.schema)
    w.load(o)
    with aclgpu.Engine(w.schema, device=0) as e:
        w.load(e)
        items = e.make_items(rt, pm, res, st, "", subj)
        perm, err, flags, off, raw = e.explain_ids(items)
        cperm, cerr = e.check_bulk_ids(items)
        operm, oerr = o.check_bulk_ids(rt, pm, res, st, "", subj)
        assert np.array_equal(perm, cperm) and np.array_equal(err, cerr)
        assert np.array_equal(perm, operm) and np.array_equal(err, oerr)
        has = (perm == PERM_HAS) & (err == 0)
        assert int(has.sum()) >= 256
        assert np.array_equal(flags, np.where(has, aclgpu.EXPLAIN_WITNESS, 0).astype(np.uint8))
        assert off[0] == 0 and off[n] == raw.size and np.all(np.diff(off.astype(np.int64)) >= 0)
        assert np.all((np.diff(off.astype(np.int64)) > 0) == has)  # (plain subjects: a granted item has hops, any other has none)
        conv = namer(e, w.schema, named=False)
        replayed = 0
        for i in np.flatnonzero(has):
            hops = conv(raw[off[i]:off[i + 1]])
            X.check_witness(w.schema, stored, (rt, str(int(res[i])), pm, st, str(int(subj[i])), ""), hops, replay_it=replayed < 256)
            replayed += 1


# ---------------------------------------------------------------- 4. non-monotone permissions in a mixed batch
def test_non_monotone_items_are_answered_not_explained(aclgpu):
    schema = """
definition user {}
definition doc {
  relation viewer: user
  relation banned: user
  relation editor: user
  permission view = viewer - banned
  permission edit = editor
}
"""
    rels = [("doc", "d", "viewer", "user", "a", ""), ("doc", "d", "viewer", "user", "b", ""), ("doc", "d", "banned", "user", "b", ""), ("doc", "d", "editor", "user", "a", "")]
    named = [("doc", "d", "view", "user", "a", ""), ("doc", "d", "edit", "user", "a", ""), ("doc", "d", "view", "user", "b", ""), ("doc", "d", "edit", "user", "b", ""),
             ("doc", "d", "view", "user", "a", ""), ("doc", "d", "edit", "user", "a", "")]
    with aclgpu.Engine(schema, device=0) as e:
        e.touch(*rels)
        items = np.concatenate([item_ids(e, it) for it in named])
        perm, err, flags, off, raw = e.explain_ids(items)  # (returns: the call is ACL_OK)
        cperm, cerr = e.check_bulk_ids(items)
        assert np.array_equal(perm, cperm) and np.array_equal(err, cerr)
        assert perm.tolist() == [PERM_HAS, PERM_HAS, PERM_NO, PERM_NO, PERM_HAS, PERM_HAS] and not err.any()
        assert flags.tolist() == [aclgpu.EXPLAIN_UNSUPPORTED, aclgpu.EXPLAIN_WITNESS, 0, 0, aclgpu.EXPLAIN_UNSUPPORTED, aclgpu.EXPLAIN_WITNESS]
        assert off.tolist() == [0, 0, 1, 1, 1, 1, 2]
        conv = namer(e, schema)
        for i in (1, 5):
            X.check_witness(schema, set(rels), named[i], conv(raw[off[i]:off[i + 1]]))
        p, er, fl, lines = e.explain(*named[0])
        assert (p, er, fl, lines) == (PERM_HAS, 0, aclgpu.EXPLAIN_UNSUPPORTED, [])


# ---------------------------------------------------------------- 5. a level wider than the first log region
def test_overflow_retry(aclgpu, C4):
    n = 20000
    with aclgpu.Engine(C4, device=0) as e:
        e.add_edges("group", "member", "group", "member", np.zeros(n, dtype=np.uint32), np.arange(1, n + 1, dtype=np.uint32))
        e.add_edges("group", "member", "user", "", [n], [0])
        e.add_edges("pod", "viewer", "group", "member", [0], [0])
        items = e.make_items("pod", "view", [0], "user", "", [0])
        perm, err = e.check_bulk_ids(items)
        assert (int(perm[0]), int(err[0])) == (PERM_HAS, 0)
        s0 = e.stats()["overflow_retries"]
        e.check_bulk_ids(items)
        s1 = e.stats()["overflow_retries"]
        perm, err, flags, off, raw = e.explain_ids(items)
        assert (int(perm[0]), int(err[0]), int(flags[0])) == (PERM_HAS, 0, aclgpu.EXPLAIN_WITNESS)
        assert e.stats()["overflow_retries"] - s1 > s1 - s0  # (more than the Check inside the call accounts for: the walk's own region was redone)
        hops = namer(e, C4, named=False)(raw)
        want = [("pod", "0", "viewer", "group", "0", "member"), ("group", "0", "member", "group", str(n), "member"), ("group", str(n), "member", "user", "0", "")]
        assert hops == want
        X.check_witness(C4, set(want), ("pod", "0", "view", "user", "0", ""), hops)


# ---------------------------------------------------------------- 6. writes and time
def test_deleting_a_hop_moves_the_witness(aclgpu, C4):
    item = ("pod", "p", "view", "user", "u", "")
    rels = [("pod", "p", "viewer", "group", "a", "member"), ("group", "a", "member", "group", "c", "member"), ("group", "c", "member", "user", "u", ""),
            ("pod", "p", "viewer", "group", "b", "member"), ("group", "b", "member", "group", "d", "member"), ("group", "d", "member", "user", "u", "")]
    with aclgpu.Engine(C4, device=0) as e:
        e.touch(*rels)
        live = list(rels)
        _, _, fl, first = explain_both(aclgpu, e, C4, live, item, exact=False)
        assert fl == aclgpu.EXPLAIN_WITNESS and len(first) == 3
        e.write([(aclgpu.OP_DELETE, first[1])])
        live.remove(first[1])
        _, _, fl, second = explain_both(aclgpu, e, C4, live, item)  # (held to the checker against what is stored NOW)
        assert fl == aclgpu.EXPLAIN_WITNESS and len(second) == 3 and not set(second) & set(first)
        e.write([(aclgpu.OP_DELETE, second[1])])
        live.remove(second[1])
        p, er, fl, hops = explain_both(aclgpu, e, C4, live, item)
        assert (p, er, fl, hops) == (PERM_NO, 0, 0, [])


def test_an_expired_hop_is_no_witness(aclgpu):
    schema = """
definition user {}
definition group {
  relation member: user | group#member
}
definition pod {
  relation viewer: user with expiration | group#member
  permission view = viewer
}
"""
    item = ("pod", "p", "view", "user", "u", "")
    direct = ("pod", "p", "viewer", "user", "u", "")
    long = [("pod", "p", "viewer", "group", "g", "member"), ("group", "g", "member", "user", "u", "")]
    with aclgpu.Engine(schema, device=0) as e:
        e.set_now(100)
        e.touch(*long)
        e.write([(aclgpu.OP_TOUCH, direct, 1000)])
        _, _, fl, hops = explain_both(aclgpu, e, schema, long + [direct], item)
        assert fl == aclgpu.EXPLAIN_WITNESS and hops == [direct]
        e.set_now(1000)  # the direct grant has run out
        _, _, fl, hops = explain_both(aclgpu, e, schema, long, item)
        assert fl == aclgpu.EXPLAIN_WITNESS and hops == long
        e.write([(aclgpu.OP_DELETE, long[1])])
        p, er, fl, hops = explain_both(aclgpu, e, schema, long[:1], item)
        assert (p, er, fl, hops) == (PERM_NO, 0, 0, [])


# ---------------------------------------------------------------- 7. shapes
def test_batch_shapes(aclgpu, C4):
    rels = [("pod", "p", "viewer", "group", "g", "member"), ("group", "g", "member", "user", "u", ""), ("pod", "q", "creator", "user", "v", ""),
            ("pod", "q", "namespace", "namespace", "n", ""), ("namespace", "n", "viewer", "user", "u", "")]
    named = [("pod", "p", "view", "user", "u", ""), ("pod", "q", "view", "user", "v", ""), ("pod", "q", "view", "user", "u", ""), ("pod", "p", "view", "user", "v", ""),
             ("namespace", "n", "view", "user", "u", ""), ("pod", "p", "viewer", "group", "g", "member")]
    want = [[rels[0], rels[1]], [rels[2]], [rels[3], rels[4]], None, [rels[4]], [rels[0]]]
    with aclgpu.Engine(C4, device=0) as e:
        e.touch(*rels)
        perm, err, flags, off, raw = e.explain_ids(np.zeros(0, dtype=aclgpu.ITEM_DTYPE))  # n = 0
        assert perm.size == err.size == flags.size == raw.size == 0 and off.tolist() == [0]
        one = [item_ids(e, it) for it in named]
        conv = namer(e, C4)
        for it, ids, w in zip(named, one, want):  # n = 1, both entry points
            p, er, fl, hops = explain_both(aclgpu, e, C4, rels, it)
            assert hops == (w or []) and fl == (aclgpu.EXPLAIN_WITNESS if w is not None else 0)
        pick = np.arange(1025) % len(named)  # 1 025 items, every one many times over, types and permissions mixed
        items = np.concatenate(one)[pick]
        perm, err, flags, off, raw = e.explain_ids(items)
        cperm, cerr = e.check_bulk_ids(items)
        assert np.array_equal(perm, cperm) and np.array_equal(err, cerr) and off[-1] == raw.size
        for i, k in enumerate(pick):
            hops = conv(raw[off[i]:off[i + 1]])
            assert hops == (want[k] or []), (i, k)
            assert int(flags[i]) == (aclgpu.EXPLAIN_WITNESS if want[k] is not None else 0)
        X.check_witness(C4, set(rels), named[2], conv(raw[off[2]:off[3]]))
        # acl_call_opts_t: already cancelled / already past its deadline are refused; a live flag and a generous deadline change nothing
        flag = ctypes.c_int32(1)
        with pytest.raises(aclgpu.AclError) as x:
            e.explain_ids(items, cancel=flag)
        assert x.value.code == aclgpu.ERR_CANCELLED
        with pytest.raises(aclgpu.AclError) as x:
            e.explain_ids(items, timeout_s=1e-9)
        assert x.value.code == aclgpu.ERR_DEADLINE_EXCEEDED
        flag.value = 0
        again = e.explain_ids(items, cancel=flag, timeout_s=60.0)
        assert all(np.array_equal(u, v) for u, v in zip(again, (perm, err, flags, off, raw)))

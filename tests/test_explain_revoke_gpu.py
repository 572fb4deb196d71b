"""Explain for revocation on the GPU (k_revoke_local + engine_revoke.cpp) through the C ABI's Python mirror.

acl_explain_revoke*(item) = Check(item) + for every item granted on a monotone permission ALL single stored relationships whose delete takes the grant away.
Every answer goes through ONE checker (tests/revoke_checker.py), which works from the test's own relationships and both oracles: each cut is stored, each
cut deleted alone revokes the item on both oracles, and no other relationship of the store does (the C oracle's brute force over the whole store; the Python
oracle repeats it for the hops of a validated witness).

The brute force of one random graph (all relationships x all granted items, the oracles alone, one CPU core): 1.1 to 2.6 s for the eight seeds, 380
relationships and 880 to 1 220 granted items each (seed 0: 2.55 s, 1: 2.13, 2: 1.38, 5: 1.83, 6: 1.13, 8: 1.76, 10: 1.63, 12: 1.68)."""
import ctypes
import random

import numpy as np
import pytest

from tests import explain_checker as X
from tests import revoke_checker as R
from tests.test_explain_denial_gpu import engine, ids_of, load_by_ids
from tests.test_explain_gpu import depth_graph, namer

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


def revoke_both(aclgpu, e, ck, item, named=True, sample=None):
    """one named item through BOTH entry points: they agree with each other and with Check; a granted monotone item's cuts go through the checker, with a
    witness taken from explain_ids on the same engine and validated first.  -> (perm, err, flags, cuts as 6-tuples in the ids form's order, witness)"""
    from aclgpu.text import parse_relationship
    schema = ck.orcs.schema
    ids = ids_of(e, [item]) if named else e.make_items(item[0], item[2], [int(item[1])], item[3], item[5], [int(item[4])])  # (loaded by id: the names ARE the ids)
    perm, err, flags, off, raw = e.explain_revoke_ids(ids)
    cperm, cerr = e.check_bulk_ids(ids)
    p, er, fl = int(perm[0]), int(err[0]), int(flags[0])
    assert (p, er) == (int(cperm[0]), int(cerr[0])) and off.tolist() == [0, raw.size]
    cuts = namer(e, schema, named=named)(raw)
    if named:
        sp, ser, sfl, lines = e.explain_revoke(*item)
        assert (sp, ser, sfl) == (p, er, fl) == e.check(*item) + (fl,)
        text = [parse_relationship(ln) for ln in lines]
        assert len(text) == len(cuts) and set(text) == set(cuts)
    witness = None
    if fl & aclgpu.EXPLAIN_REVOKE:
        assert (p, er, fl) == (PERM_HAS, 0, aclgpu.EXPLAIN_REVOKE)
        _, _, wfl, _, wraw = e.explain_ids(ids)
        assert int(wfl[0]) == aclgpu.EXPLAIN_WITNESS
        witness = namer(e, schema, named=named)(wraw)
        X.check_witness(schema, set(ck.orcs.rels), item, witness)
        ck.check(item, cuts, witness=witness, sample=sample)
        assert set(cuts) <= set(witness)
    else:
        assert cuts == []
    return p, er, fl, cuts, witness


def case(aclgpu, schema, rels, now=None):
    return R.Checker(schema, rels, now or 0), engine(aclgpu, schema, rels, now)


# ---------------------------------------------------------------- 1. hand graphs
def test_every_hop_of_one_chain_is_a_cut_in_chain_order(aclgpu, C4):
    chain = [("pod", "ns/a", "namespace", "namespace", "ns", ""), ("namespace", "ns", "viewer", "group", "g", "member"), ("group", "g", "member", "user", "u", "")]
    rels = chain + [("pod", "ns/a", "viewer", "user", "other", ""), ("group", "g", "member", "user", "other", ""), ("namespace", "ns", "creator", "user", "other", "")]
    ck, e = case(aclgpu, C4, rels)
    with e:
        p, er, fl, cuts, _ = revoke_both(aclgpu, e, ck, ("pod", "ns/a", "view", "user", "u", ""))
        assert (p, er, fl) == (PERM_HAS, 0, aclgpu.EXPLAIN_REVOKE) and cuts == chain  # arrow, userset, direct: the resource's end first
        assert e.explain_revoke("pod", "ns/a", "view", "user", "u")[3] == ["pod:ns/a#namespace@namespace:ns", "namespace:ns#viewer@group:g#member", "group:g#member@user:u"]
        p, er, fl, cuts, _ = revoke_both(aclgpu, e, ck, ("pod", "ns/a", "view", "user", "nobody", ""))
        assert (p, er, fl, cuts) == (PERM_NO, 0, 0, [])


def test_diamond_shared_ends_are_cuts_the_middles_are_not(aclgpu, C4):
    first, last = ("pod", "p", "viewer", "group", "top", "member"), ("group", "low", "member", "user", "u", "")
    rels = [first, ("group", "top", "member", "group", "l", "member"), ("group", "top", "member", "group", "r", "member"),
            ("group", "l", "member", "group", "low", "member"), ("group", "r", "member", "group", "low", "member"), last]
    ck, e = case(aclgpu, C4, rels)
    with e:
        _, _, fl, cuts, witness = revoke_both(aclgpu, e, ck, ("pod", "p", "view", "user", "u", ""))
        assert fl == aclgpu.EXPLAIN_REVOKE and cuts == [first, last] and len(witness) == 4


def test_two_disjoint_chains_have_no_cut(aclgpu, C4):
    rels = [("pod", "p", "viewer", "group", "a", "member"), ("group", "a", "member", "user", "u", ""),
            ("pod", "p", "namespace", "namespace", "n", ""), ("namespace", "n", "viewer", "group", "b", "member"), ("group", "b", "member", "user", "u", "")]
    ck, e = case(aclgpu, C4, rels)
    with e:
        p, er, fl, cuts, _ = revoke_both(aclgpu, e, ck, ("pod", "p", "view", "user", "u", ""))
        assert (p, er, fl, cuts) == (PERM_HAS, 0, aclgpu.EXPLAIN_REVOKE, [])


def test_direct_grant_beside_a_group_route_has_no_cut(aclgpu, C4):
    rels = [("pod", "p", "viewer", "user", "u", ""), ("pod", "p", "viewer", "group", "g", "member"), ("group", "g", "member", "user", "u", "")]
    ck, e = case(aclgpu, C4, rels)
    with e:
        p, er, fl, cuts, _ = revoke_both(aclgpu, e, ck, ("pod", "p", "view", "user", "u", ""))
        assert (p, er, fl, cuts) == (PERM_HAS, 0, aclgpu.EXPLAIN_REVOKE, [])
        _, _, fl, cuts, _ = revoke_both(aclgpu, e, ck, ("pod", "p", "view", "group", "g", "member"))  # the group itself holds it by one relationship
        assert fl == aclgpu.EXPLAIN_REVOKE and cuts == [rels[1]]


# ---------------------------------------------------------------- 2. one relationship, many ops
MANY_OPS = """
definition user {}
definition group {
  relation member: user
}
definition pod {
  relation viewer: user | group#member
  permission edit = viewer
  permission view = viewer + edit
}
"""


def test_one_relationship_read_by_several_ops_is_one_cut(aclgpu):
    lone = ("pod", "p", "viewer", "user", "a", "")
    ck, e = case(aclgpu, MANY_OPS, [lone, ("pod", "p", "viewer", "user", "b", "")])
    with e:
        for perm in ("view", "edit"):
            _, _, fl, cuts, _ = revoke_both(aclgpu, e, ck, ("pod", "p", perm, "user", "a", ""))
            assert fl == aclgpu.EXPLAIN_REVOKE and cuts == [lone]
    # a second route that grants `viewer`: the lone relationship is no cut any more, and neither is anything else
    ck, e = case(aclgpu, MANY_OPS, [lone, ("pod", "p", "viewer", "group", "g", "member"), ("group", "g", "member", "user", "a", "")])
    with e:
        _, _, fl, cuts, _ = revoke_both(aclgpu, e, ck, ("pod", "p", "view", "user", "a", ""))
        assert fl == aclgpu.EXPLAIN_REVOKE and cuts == []


# ---------------------------------------------------------------- 3. wildcards
WILD = """
definition user {}
definition group {
  relation member: user | group#member
}
definition doc {
  relation viewer: user | user:* | group#member
  permission view = viewer
}
"""


def test_wildcard_relationship_is_the_cut_and_carries_the_flag(aclgpu):
    star = ("doc", "open", "viewer", "user", "*", "")
    ck, e = case(aclgpu, WILD, [star, ("doc", "other", "viewer", "user", "u", "")])
    with e:
        item = ("doc", "open", "view", "user", "u", "")
        _, _, fl, cuts, _ = revoke_both(aclgpu, e, ck, item)
        assert fl == aclgpu.EXPLAIN_REVOKE and cuts == [star]
        raw = e.explain_revoke_ids(ids_of(e, [item]))[4]
        assert int(raw[0]["flags"]) == aclgpu.HOP_WILDCARD and int(raw[0]["sid"]) == e.find("user", "*")
        assert e.explain_revoke(*item)[3] == ["doc:open#viewer@user:*"]
    ck, e = case(aclgpu, WILD, [star, ("doc", "open", "viewer", "user", "u", ""), ("doc", "open", "viewer", "user", "v", "")])
    with e:  # `user:*` beside the named user: neither alone takes it away; for anybody else the wildcard still does
        _, _, fl, cuts, _ = revoke_both(aclgpu, e, ck, ("doc", "open", "view", "user", "u", ""))
        assert fl == aclgpu.EXPLAIN_REVOKE and cuts == []
        ck.orcs.touch_all([("doc", "x", "viewer", "user", "w", "")])
        e.touch(("doc", "x", "viewer", "user", "w", ""))
        _, _, fl, cuts, _ = revoke_both(aclgpu, e, ck, ("doc", "open", "view", "user", "w", ""))
        assert fl == aclgpu.EXPLAIN_REVOKE and cuts == [star]


# ---------------------------------------------------------------- 4. a subject with a relation
def test_subject_with_a_relation(aclgpu, C4):
    rels = [("pod", "p", "viewer", "group", "g", "member"), ("group", "g", "member", "user", "u", ""), ("group", "g", "member", "group", "h", "member"),
            ("pod", "q", "viewer", "group", "g", "member"), ("pod", "q", "viewer", "group", "k", "member"), ("group", "k", "member", "group", "h", "member")]
    ck, e = case(aclgpu, C4, rels)
    with e:
        _, _, fl, cuts, _ = revoke_both(aclgpu, e, ck, ("pod", "p", "view", "group", "g", "member"))
        assert fl == aclgpu.EXPLAIN_REVOKE and cuts == [rels[0]]
        # g's member row is probed for h#member and enumerated for its children at once: the one relationship is left out of both
        _, _, fl, cuts, _ = revoke_both(aclgpu, e, ck, ("pod", "p", "view", "group", "h", "member"))
        assert fl == aclgpu.EXPLAIN_REVOKE and cuts == [rels[0], rels[2]]
        _, _, fl, cuts, _ = revoke_both(aclgpu, e, ck, ("pod", "q", "view", "group", "h", "member"))  # through g and through k
        assert fl == aclgpu.EXPLAIN_REVOKE and cuts == []
        # the reflexive item is granted by zero hops: nothing to delete
        p, er, fl, cuts, witness = revoke_both(aclgpu, e, ck, ("group", "g", "member", "group", "g", "member"))
        assert (p, er, fl, cuts, witness) == (PERM_HAS, 0, aclgpu.EXPLAIN_REVOKE, [], [])


# ---------------------------------------------------------------- 5. the depth limit
def test_depth_limit(aclgpu, C4):
    item = ("pod", "p", "view", "user", "u", "")
    short = [("pod", "p", "viewer", "group", "s0", "member"), ("group", "s0", "member", "user", "u", "")]
    # the second chain's Check ends exactly at level 50 (tests/test_explain_gpu.py: 49 hops): it keeps the grant alive when a hop of the short one goes
    long = depth_graph(47)
    ck, e = case(aclgpu, C4, short + long)
    with e:
        p, er, fl, cuts, witness = revoke_both(aclgpu, e, ck, item)
        assert (p, er, fl, cuts) == (PERM_HAS, 0, aclgpu.EXPLAIN_REVOKE, []) and witness == short
    ck, e = case(aclgpu, C4, long)
    with e:  # ... and on its own all of its 49 hops are cuts
        _, _, fl, cuts, _ = revoke_both(aclgpu, e, ck, item)
        assert fl == aclgpu.EXPLAIN_REVOKE and cuts == long
    # one level longer: the chain that is left answers ACL_ERR_DEPTH, which is not HAS -- the short chain's hops are cuts
    ck, e = case(aclgpu, C4, short + depth_graph(48))
    with e:
        _, _, fl, cuts, _ = revoke_both(aclgpu, e, ck, item)
        assert fl == aclgpu.EXPLAIN_REVOKE and cuts == short
        e.write([(aclgpu.OP_DELETE, short[1])])
        assert e.check(*item)[1] == aclgpu.ERR_DEPTH and e.explain_revoke(*item)[1:] == (aclgpu.ERR_DEPTH, 0, [])


# ---------------------------------------------------------------- 6. a closure wider than the first log region
def test_masked_walks_run_the_closure_dry_through_the_redo(aclgpu, C4):
    n = 17000
    chain = [("pod", "0", "viewer", "group", "0", "member"), ("group", "0", "member", "group", str(n), "member"), ("group", str(n), "member", "user", "0", "")]
    rels = chain[:1] + [("group", "0", "member", "group", str(i), "member") for i in range(1, n + 1)] + chain[2:]
    ck = R.Checker(C4, rels)
    with aclgpu.Engine(C4, device=0) as e:
        load_by_ids(e, rels)
        items = e.make_items("pod", "view", [0], "user", "", [0])
        for _ in range(3):  # (the snapshot and whatever the Check learns about this graph on its first calls are behind us)
            e.explain_ids(items)
        s0 = e.stats()["overflow_retries"]
        e.explain_ids(items)
        s1 = e.stats()["overflow_retries"]
        perm, err, flags, off, raw = e.explain_revoke_ids(items)
        moved = (e.stats()["overflow_retries"] - s1) - (s1 - s0)  # (beyond what the Check and the witness walk inside the call account for)
        print(f"overflow_retries: Explain moves {s1 - s0}, the masked walks moved {moved} more")
        assert (int(perm[0]), int(err[0]), int(flags[0])) == (PERM_HAS, 0, aclgpu.EXPLAIN_REVOKE)
        assert namer(e, C4, named=False)(raw) == chain
        assert moved >= 1  # the walks that leave out the second and the third hop hold 17 000 states: beyond the first region of 16 384
        p, er, fl, cuts, _ = revoke_both(aclgpu, e, ck, ("pod", "0", "view", "user", "0", ""), named=False, sample=100)
        assert cuts == chain


# ---------------------------------------------------------------- 7. one call of 300 items
MIXED = R.NESTED.replace("  permission view = viewer + edit + folder->view\n", """  permission view = viewer + edit + folder->view
  relation banned: user
  permission safe = view - banned
  permission both = viewer & editor
  permission every = folder.all(view)
""")
MONOTONE = {("doc", "view"), ("doc", "edit"), ("folder", "view"), ("group", "member")}


def mixed_batch():
    """(Checker over MIXED, 299 named items): granted and denied items of a random graph, all three kinds of non-monotone permission, two depth errors,
    a reflexive item, several resource types and subject classes"""
    assert "permission every" in MIXED
    rels, cand = R.random_graph(3)
    rels += [("doc", "x", "viewer", "user", "u0", ""), ("doc", "x", "editor", "user", "u0", ""), ("doc", "x", "folder", "folder", "fx", ""),
             ("folder", "fx", "viewer", "user", "u0", ""), ("doc", "x", "banned", "user", "u1", ""), ("doc", "x", "viewer", "user", "u1", "")]
    rels += [("doc", "deep", "viewer", "group", "c0", "member")] + [("group", f"c{i}", "member", "group", f"c{i + 1}", "member") for i in range(60)]
    rels += [("group", "c60", "member", "user", "deepuser", "")]
    ck = R.Checker(MIXED, rels)
    rnd = random.Random(300)
    granted = [it for it in cand if ck.granted(it)]
    denied = [it for it in cand if it not in set(granted)]
    items = rnd.sample(granted, 170) + rnd.sample(denied, 80)
    items += [("doc", "x", pm, "user", u, "") for pm in ("safe", "both", "every", "view", "edit") for u in ("u0", "u1", "u2")]
    items += [(it[0], it[1], "safe", *it[3:]) for it in granted[:12] if it[0] == "doc" and it[2] == "view" and not it[5]]
    items += [("group", "g0", "member", "group", "g0", "member"), ("group", "c0", "member", "user", "deepuser", ""), ("doc", "deep", "view", "user", "deepuser", ""),
              ("doc", "deep", "view", "user", "u0", ""), ("folder", "fx", "view", "user", "u0", "")]
    items += rnd.sample(granted, 299 - len(items))
    rnd.shuffle(items)
    return ck, items, granted


def test_three_hundred_items_in_one_call(aclgpu, aclgpu_lib):
    ck, items, granted = mixed_batch()
    rnd = random.Random(301)
    with engine(aclgpu, MIXED, ck.orcs.rels) as e:
        ids = ids_of(e, items)
        bad = ids_of(e, granted[:1])
        bad["permission"] = 77  # an unknown permission: the item's own error
        ids = np.concatenate([ids[:150], bad, ids[150:]])
        items = items[:150] + [None] + items[150:]
        assert len(items) == 300
        perm, err, flags, off, raw = e.explain_revoke_ids(ids)
        cperm, cerr = e.check_bulk_ids(ids)
        assert np.array_equal(perm, cperm) and np.array_equal(err, cerr)
        assert off[0] == 0 and off[-1] == raw.size and np.all(np.diff(off.astype(np.int64)) >= 0)
        conv = namer(e, MIXED)
        seen = {"cut": 0, "none": 0, "unsupported": 0, "denied": 0, "error": 0}
        for i, it in enumerate(items):
            cuts = conv(raw[off[i]:off[i + 1]])
            if it is None:
                assert int(err[i]) != 0 and int(flags[i]) == 0 and cuts == []
                seen["error"] += 1
                continue
            (op, oe), oy = ck.orcs.check(it)
            assert (int(perm[i]), int(err[i])) == (op, oe), it
            if oe or op != PERM_HAS:
                assert int(flags[i]) == 0 and cuts == [], it
                seen["error" if oe else "denied"] += 1
            elif (it[0], it[2]) not in MONOTONE:
                assert int(flags[i]) == aclgpu.EXPLAIN_UNSUPPORTED and cuts == [], it
                seen["unsupported"] += 1
            else:
                assert int(flags[i]) == aclgpu.EXPLAIN_REVOKE, it
                ck.check(it, cuts)
                seen["cut" if cuts else "none"] += 1
        print(seen)
        assert seen["error"] >= 2 and seen["unsupported"] >= 6 and seen["denied"] >= 80 and seen["cut"] >= 40 and seen["none"] >= 20
        assert int(err[items.index(("doc", "deep", "view", "user", "deepuser", ""))]) == aclgpu.ERR_DEPTH
        # every item once more through both entry points, with its witness, for a sample; and the same call again: the same sets
        for it in rnd.sample([it for it in items if it is not None], 24):
            revoke_both(aclgpu, e, ck, it)
        again = e.explain_revoke_ids(ids)
        assert all(np.array_equal(u, v) for u, v in zip(again[:4], (perm, err, flags, off)))
        for i in range(300):
            assert set(conv(again[4][off[i]:off[i + 1]])) == set(conv(raw[off[i]:off[i + 1]]))
        # n == 0
        perm, err, flags, off, raw = e.explain_revoke_ids(np.zeros(0, dtype=aclgpu.ITEM_DTYPE))
        assert perm.size == err.size == flags.size == raw.size == 0 and off.tolist() == [0]
        # acl_call_opts_t: already cancelled / already past its deadline are refused; a live flag and a generous deadline change nothing
        flag = ctypes.c_int32(1)
        with pytest.raises(aclgpu.AclError) as x:
            e.explain_revoke_ids(ids, cancel=flag)
        assert x.value.code == aclgpu.ERR_CANCELLED
        with pytest.raises(aclgpu.AclError) as x:
            e.explain_revoke_ids(ids, timeout_s=1e-9)
        assert x.value.code == aclgpu.ERR_DEADLINE_EXCEEDED
        flag.value = 0
        once_more = e.explain_revoke_ids(ids, cancel=flag, timeout_s=60.0)
        assert all(np.array_equal(u, v) for u, v in zip(once_more[:4], again[:4])) and once_more[4].size == again[4].size
        # one shard of a sharded graph does not explain
        e._check(aclgpu_lib.acl_shard_configure(e._h, 0, 2))
        with pytest.raises(aclgpu.AclError) as x:
            e.explain_revoke_ids(ids)
        assert x.value.code == aclgpu.ERR_FAILED_PRECONDITION
        with pytest.raises(aclgpu.AclError) as x:
            e.explain_revoke("doc", "x", "view", "user", "u0")
        assert x.value.code == aclgpu.ERR_FAILED_PRECONDITION


# ---------------------------------------------------------------- 8. random graphs with nested groups and arrows
@pytest.mark.parametrize("seed", R.SEEDS)
def test_random_graphs(aclgpu, seed):
    ck, granted, want = R.random_case(seed)  # (the brute force and the conditions on the graph: the oracle side, before the engine is asked)
    with engine(aclgpu, R.NESTED, ck.orcs.rels) as e:
        ids = ids_of(e, granted)
        perm, err, flags, off, raw = e.explain_revoke_ids(ids)
        assert np.all(perm == PERM_HAS) and not err.any() and np.all(flags == aclgpu.EXPLAIN_REVOKE)
        conv = namer(e, R.NESTED)
        for i, it in enumerate(granted):
            cuts = conv(raw[off[i]:off[i + 1]])
            assert set(cuts) == want[it] and len(cuts) == len(want[it]), (it, cuts, sorted(want[it]))
            ck.check(it, cuts)
        for it in random.Random(seed).sample(granted, 16):  # both entry points, the witness and the Python oracle's share
            revoke_both(aclgpu, e, ck, it)


# ---------------------------------------------------------------- 9. after a write
def test_deleting_a_cut_revokes_and_touching_it_back_restores_the_set(aclgpu, C4):
    item = ("pod", "p", "view", "user", "u", "")
    rels = [("pod", "p", "namespace", "namespace", "n", ""), ("namespace", "n", "viewer", "group", "a", "member"), ("namespace", "n", "viewer", "group", "b", "member"),
            ("group", "a", "member", "group", "c", "member"), ("group", "b", "member", "group", "c", "member"), ("group", "c", "member", "user", "u", "")]
    ck, e = case(aclgpu, C4, rels)
    with e:
        _, _, fl, first, _ = revoke_both(aclgpu, e, ck, item)
        assert fl == aclgpu.EXPLAIN_REVOKE and first == [rels[0], rels[5]]
        for cut in first:
            e.write([(aclgpu.OP_DELETE, cut)])
            p, er = e.check(*item)
            assert p != PERM_HAS
            assert e.explain_revoke(*item) == (p, er, 0, [])
            e.write([(aclgpu.OP_TOUCH, cut)])
            _, _, fl, cuts, _ = revoke_both(aclgpu, e, ck, item)
            assert fl == aclgpu.EXPLAIN_REVOKE and set(cuts) == set(first)
        # a delete that is no cut leaves the grant, and makes the rest of that route cuts
        e.write([(aclgpu.OP_DELETE, rels[2])])
        ck = R.Checker(C4, [r for r in rels if r != rels[2]])
        _, _, fl, cuts, _ = revoke_both(aclgpu, e, ck, item)
        assert fl == aclgpu.EXPLAIN_REVOKE and cuts == [rels[0], rels[1], rels[3], rels[5]]

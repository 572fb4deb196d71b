"""LookupSubjects on the type-hash sharded graph (acl_shard_subjects_bulk: k_subj_expand + engine_shard_subjects.cpp), G logical shards of one GPU
through the in-process ThreadNative communicator -- the loop, the kernels and the decisions are the ones RCCL drives.

Expected values come from the oracles' Check (tests/test_lookup_subjects_gpu.py contract / check_rows), never from the engine under test; every rank's
output is asserted.  Shard placements (plan.cpp shard_of_type): C4 -- world 2: pod 0, group + namespace 1; world 5: pod + group 4, namespace 3; world 8:
pod 4, group 1, namespace 3.  team / crew -- world 3: team 1, crew 0.  SCHEMA_CHAIN -- world 2: doc 0, group 1; world 3: doc 2, group 0.
SCHEMA_WILD -- world 8: doc 2, group 1, folder 6."""
import numpy as np
import pytest

from oracle import orc
from oracle.pyoracle import MAX_DEPTH
from tests.test_lookup_subjects_gpu import SCHEMA_CHAIN, SCHEMA_WILD, WILD_RELS, check_rows, contract, ids_of
from tests.test_sharded_gloo import CHAIN_SCHEMA, chain_case

pytestmark = pytest.mark.gpu

PERM_HAS = 2
EMPTY_POD = "no-relationships-at-all"


@pytest.fixture(scope="module")
def aclgpu(aclgpu_lib):
    import aclgpu as m
    return m


def run_shards(aclgpu, world, schema, load, fn, **engine_kw):
    """one Engine(schema, contexts=1) per rank, loaded identically by load(engine); fn(ShardedEngine) on every rank -> the per-rank results"""
    from aclgpu import sharded
    engines = []

    def make(rank, nshards):
        e = aclgpu.Engine(schema, contexts=1, **engine_kw)
        load(e)
        engines.append(e)
        return sharded.GpuShard(e, rank, nshards)

    try:
        return sharded.run_logical_shards(world, make, fn)
    finally:
        for e in engines:
            e.close()


def answer(aclgpu, se, rt, rid, perm, st, srel="", want_excluded=True):
    """the string form of one lookup through the native loop: (names, wildcard, excluded names) or "DEPTH" """
    e = se.shard.e
    try:
        bm, flags, ex, stats = se.lookup_subjects_ids_batch_native(rt, perm, st, srel, [e.find(rt, rid)], want_excluded=want_excluded)
    except aclgpu.AclError as x:
        if x.code == aclgpu.ERR_DEPTH:
            return "DEPTH"
        raise
    wild = bool(flags[0] & 1)
    names = set(e.bitmap_names(st, bm[0].cpu().numpy().view(np.uint32)))
    excl = set(e.bitmap_names(st, ex[0].cpu().numpy().view(np.uint32))) if (ex is not None and wild) else set()
    return names, wild, excl


def names_of(rels, st):
    """every name of the subject type the relationships mention but the wildcard's own (what subjects_of_type reads off an engine)"""
    out = []
    for r in rels:
        for t, n in ((r[0], r[1]), (r[3], r[4])):
            if t == st and n != "*" and n not in out:
                out.append(n)
    return out


# ---------------------------------------------------------------------------------------------------------------- 1, 2, 6, 7: C4
@pytest.fixture(scope="module")
def c4_case():
    """C4 at a small scale: 63 random pods, pod 0, a pod whose row holds users that ONLY pod#creator, ONLY a group and ONLY namespace#creator give (each
    marked by a different shard at world 8, into the same row: the case a byte-wise max would get wrong), and one interned pod without relationships.
    The expected rows are computed once, by the C oracle's Check over R x U, and shared by the tests below (never modified)."""
    from aclgpu import workloads
    w = workloads.c4(scale=0.01, n_user=2000)
    o = orc.Oracle(w.schema)
    w.load(o)
    E = {(e[0], e[1], e[2]): (e[4], e[5]) for e in w.edges}
    pod_ns, pod_creator, ns_creator = E[("pod", "namespace", "namespace")][1], E[("pod", "creator", "user")][1], E[("namespace", "creator", "user")][1]
    pvu_r, pvu_s = E[("pod", "viewer", "user")]
    pvg_r, nvg_r = E[("pod", "viewer", "group")][0], E[("namespace", "viewer", "group")][0]
    npod, nuser, ngroup = w.nobjects["pod"], w.nobjects["user"], w.nobjects["group"]
    users = np.arange(nuser, dtype=np.uint32)

    def has(rt, rel, rid):
        p, _ = o.check_bulk_ids_mt(8, rt, rel, np.full(nuser, rid, dtype=np.uint32), "user", "", users)
        return p == PERM_HAS

    # candidates by the arrays (a pod with a group viewer in a namespace without one), confirmed by the oracle
    mixed = None
    ns_without_groups = np.setdiff1d(np.arange(w.nobjects["namespace"]), nvg_r)
    for p in np.flatnonzero(np.isin(pod_ns, ns_without_groups) & np.isin(np.arange(npod), pvg_r))[:200]:
        ns, c, nc = int(pod_ns[p]), int(pod_creator[p]), int(ns_creator[pod_ns[p]])
        pv, nv = has("pod", "viewer", p), has("namespace", "viewer", ns)
        direct = np.zeros(nuser, dtype=bool)
        direct[pvu_s[pvu_r == p]] = True
        only_group = pv & ~direct & ~nv
        only_group[[c, nc]] = False
        if c != nc and not pv[c] and not nv[c] and not pv[nc] and not nv[nc] and only_group.any():
            mixed = (int(p), c, nc, int(np.flatnonzero(only_group)[0]))
            break
    assert mixed is not None, "no pod of the workload has creator-only, group-only and namespace-creator-only users"
    rids = np.unique(np.concatenate([np.random.default_rng(11).choice(npod, size=63, replace=False), [0]]).astype(np.uint32))
    rids = np.append(rids, [np.uint32(mixed[0]), np.uint32(npod)])  # (the empty pod is interned last: id npod)
    o.intern("pod", EMPTY_POD)
    want_user = check_rows(o, "pod", "view", rids, "user", "", nuser)
    want_group = check_rows(o, "pod", "view", rids, "group", "member", ngroup)
    assert sum(len(x) for x in want_user) > 0 and sum(len(x) for x in want_group) > 0
    assert not want_user[-1] and not want_group[-1]
    assert {mixed[1], mixed[2], mixed[3]} <= want_user[-2]
    return {"w": w, "o": o, "rids": rids, "want_user": want_user, "want_group": want_group, "mixed": mixed}


def load_c4(case):
    def load(e):
        case["w"].load(e)
        assert e.intern("pod", EMPTY_POD) == int(case["rids"][-1])
    return load


def rows_of(t):
    return t.cpu().numpy().view(np.uint32)


def assert_rows(got, want, what):
    assert got.shape[0] == len(want)
    for i, ids in enumerate(want):
        assert ids_of(got[i]) == ids, (what, i)


@pytest.mark.parametrize("world", [2, 5, 8])
def test_c4_parity(aclgpu, c4_case, world):
    """(pod, view, user) and (pod, view, group#member) equal {s : Check == HAS} on every rank; entries crossed shards; the second identical call
    returns the same rows with one synchronisation per burst plus the final one."""
    rids = c4_case["rids"]

    def run(se):
        b1, f1, _x, s1 = se.lookup_subjects_ids_batch_native("pod", "view", "user", "", rids)
        b2, f2, _x, s2 = se.lookup_subjects_ids_batch_native("pod", "view", "user", "", rids)
        b3, f3, _x, s3 = se.lookup_subjects_ids_batch_native("pod", "view", "group", "member", rids)
        return rows_of(b1), f1, s1, rows_of(b2), f2, s2, rows_of(b3), f3, s3

    outs = run_shards(aclgpu, world, c4_case["w"].schema, load_c4(c4_case), run)
    assert len(outs) == world
    for b1, f1, s1, b2, f2, s2, b3, f3, s3 in outs:
        print(f"world {world}: first call {s1}, second call {s2}, group#member {s3}")
        assert_rows(b1, c4_case["want_user"], "user")
        assert_rows(b3, c4_case["want_group"], "group#member")
        assert not f1.any() and not f2.any() and not f3.any()
        assert not b1[-1].any() and not b3[-1].any()  # the pod without relationships
        assert s1["entries_exchanged"] > 0 and s3["entries_exchanged"] > 0
        assert np.array_equal(b1, b2) and s2["levels"] == s1["levels"]
        assert s2["host_syncs"] <= 3  # (one chunk of lookups: one per burst -- sized by the first call's depth -- plus the final one)
        assert s1["levels"] == outs[0][2]["levels"]


def test_grow_and_redo(aclgpu, c4_case, monkeypatch):
    """A first export block of 8 entries: every shard takes the same overflow verdict, grows and redoes the chunk."""
    monkeypatch.setenv("ACL_SHARD_XCAP", "8")
    rids = c4_case["rids"]

    def run(se):
        b, f, _x, s = se.lookup_subjects_ids_batch_native("pod", "view", "user", "", rids)
        return rows_of(b), f, s

    for b, f, s in run_shards(aclgpu, 5, c4_case["w"].schema, load_c4(c4_case), run):
        print(f"xcap 8: {s}")
        assert_rows(b, c4_case["want_user"], "user")
        assert not f.any()
        assert s["retries"] >= 1 and s["export_capacity"] > 8


def test_live_writes(aclgpu, c4_case):
    """After a parity pass at world 2: one group#member@user written and one pod#viewer@user deleted on every rank's engine; the next call reflects
    both (the subject rows are rebuilt for the new epoch)."""
    w, rids = c4_case["w"], c4_case["rids"]
    E = {(e[0], e[1], e[2]): (e[4], e[5]) for e in w.edges}
    pvu_r, pvu_s = E[("pod", "viewer", "user")]
    pvg_r, pvg_s = E[("pod", "viewer", "group")]
    # the deleted viewer: a direct user viewer of one of the pods; the new member: a user the oracle does not list for a pod one of whose viewers is the
    # group.  The oracle of the graph after both writes is loaded from the workload's arrays with that one pair added and that one pair left out.
    k = int(np.flatnonzero(np.isin(pvu_r, rids))[0])
    del_pod, del_user = int(pvu_r[k]), int(pvu_s[k])
    add = None
    for j in np.flatnonzero(np.isin(pvg_r, rids)):
        i = int(np.flatnonzero(rids == pvg_r[j])[0])
        missing = sorted(set(range(w.nobjects["user"])) - c4_case["want_user"][i])
        if missing:
            add = (int(pvg_s[j]), missing[0], i)
            break
    assert add is not None
    o2 = orc.Oracle(w.schema)
    for rt, rel, st, srel, r, sj in w.edges:
        if (rt, rel, st) == ("pod", "viewer", "user"):
            keep = np.arange(r.size) != k
            r, sj = r[keep], sj[keep]
        if (rt, rel, st) == ("group", "member", "user"):
            r, sj = np.append(r, np.uint32(add[0])), np.append(sj, np.uint32(add[1]))
        o2.add_edges(rt, rel, st, srel, r, sj)
    o2.intern("pod", EMPTY_POD)
    want_after = check_rows(o2, "pod", "view", rids, "user", "", w.nobjects["user"])
    assert add[1] in want_after[add[2]] and want_after != c4_case["want_user"]

    def load(e):  # names first (dense ids follow interning order, so name k is id k of the bulk load): the writes below go by name
        for t in ("pod", "user", "group"):
            for k in range(w.nobjects[t]):
                e.intern(t, f"{t}-{k}")
        load_c4(c4_case)(e)

    def run(se):
        e = se.shard.e
        b1, _f, _x, _s = se.lookup_subjects_ids_batch_native("pod", "view", "user", "", rids)
        e.write([(aclgpu.OP_TOUCH, ("group", f"group-{add[0]}", "member", "user", f"user-{add[1]}", "")),
                 (aclgpu.OP_DELETE, ("pod", f"pod-{del_pod}", "viewer", "user", f"user-{del_user}", ""))])
        b2, _f, _x, _s = se.lookup_subjects_ids_batch_native("pod", "view", "user", "", rids)
        return rows_of(b1), rows_of(b2)

    for b1, b2 in run_shards(aclgpu, 2, w.schema, load, run):
        assert_rows(b1, c4_case["want_user"], "before")
        assert_rows(b2, want_after, "after")


def test_world_one(aclgpu, c4_case):
    """world == 1 through ThreadNative: every collective runs once, the rows equal the oracle's."""
    rids = c4_case["rids"]

    def run(se):
        b, f, _x, s = se.lookup_subjects_ids_batch_native("pod", "view", "user", "", rids)
        return rows_of(b), f, s

    (b, f, s), = run_shards(aclgpu, 1, c4_case["w"].schema, load_c4(c4_case), run)
    assert_rows(b, c4_case["want_user"], "user")
    assert not f.any() and s["entries_exchanged"] == 0 and s["exchanges"] >= s["levels"]


# ---------------------------------------------------------------------------------------------------------------- 3: depth limit across shards
def test_depth_limit_across_shards(aclgpu):
    """team:t0 <- crew:c0 <- team:t1 ... every hop crosses shards (world 3: team 1, crew 0): `deep` is listed 49 hops below and silently absent at
    50, as orc.Oracle.check says; the (team, member) subject class is answered the same way."""
    for hops in (49, 50):
        tuples = chain_case(hops)
        co = orc.Oracle(CHAIN_SCHEMA)
        co.write([(orc.OP_TOUCH, t) for t in tuples])
        teams = names_of(tuples, "team")
        want_users = {u for u in ("deep",) if co.check("team", "t0", "member", "user", u, "")[0] == PERM_HAS}
        want_teams = {t for t in teams if co.check("team", "t0", "member", "team", t, "member")[0] == PERM_HAS}
        assert want_users == ({"deep"} if hops == 49 else set()) and "t0" in want_teams and len(want_teams) >= 10

        def run(se):
            return answer(aclgpu, se, "team", "t0", "member", "user", want_excluded=False), answer(aclgpu, se, "team", "t0", "member", "team", "member", want_excluded=False)

        for users, tms in run_shards(aclgpu, 3, CHAIN_SCHEMA, lambda e: e.write([(aclgpu.OP_TOUCH, t) for t in tuples]), run):
            assert users == (want_users, False, set()), (hops, users)
            assert tms == (want_teams, False, set()), (hops, tms)


# ---------------------------------------------------------------------------------------------------------------- 4: least level
def short_path_rels(doc, pre, tail):
    """tests/test_lookup_subjects_gpu.py test_depth_short_path_through_inlined_userset's relationships under a prefix (all tails live side by side in
    one graph: one set of engines per world): group x is reached by a long path -- a chain the walk enumerates first -- and by a short one, an inlined
    computed userset (view = viewer + edit, edit = editor); the subjects below x count from the short path's level."""
    rels = [("doc", doc, "viewer", "group", f"{pre}a0", "member")]
    rels += [("group", f"{pre}a{i}", "member", "group", f"{pre}a{i + 1}", "member") for i in range(6)]
    rels += [("group", f"{pre}a6", "member", "group", f"{pre}x", "member"), ("doc", doc, "editor", "group", f"{pre}x", "member")]
    rels += [("group", f"{pre}x", "member", "group", f"{pre}t0", "member")]
    rels += [("group", f"{pre}t{i}", "member", "group", f"{pre}t{i + 1}", "member") for i in range(tail)]
    rels += [("group", f"{pre}t{tail}", "member", "user", f"{pre}end", "")]
    return rels


CYCLE_RELS = [("doc", "cyc", "viewer", "group", "g0", "member"), ("group", "g0", "member", "group", "g1", "member"),
              ("group", "g1", "member", "group", "g2", "member"), ("group", "g2", "member", "group", "g0", "member"),
              ("group", "g0", "member", "user", "alice", ""), ("group", "g2", "member", "user", "bob", ""), ("doc", "cyc", "viewer", "user", "carol", "")]


@pytest.fixture(scope="module")
def least_level_case():
    tails = list(range(MAX_DEPTH - 8, MAX_DEPTH - 1)) + [MAX_DEPTH - 6]  # (the last one again as the "end must be listed" case: a doc of its own)
    rels, queries = [], []
    for k, tail in enumerate(tails):
        rels += short_path_rels(f"d{k}", f"k{k}_", tail)
        queries += [("doc", f"d{k}", "view", "user", ""), ("doc", f"d{k}", "deep", "user", "")]
    rels += CYCLE_RELS
    queries += [("doc", "cyc", "view", "user", ""), ("group", "g1", "member", "group", "member")]
    names = {"user": names_of(rels, "user"), "group": names_of(rels, "group")}
    want = [contract(SCHEMA_CHAIN, rels, rt, rid, perm, st, srel, names[st]) for rt, rid, perm, st, srel in queries]
    assert f"k{len(tails) - 1}_end" in want[2 * (len(tails) - 1)][0]  # the short path reaches it within the limit, the long one does not
    assert want[-2][0] == {"alice", "bob", "carol"}
    assert any(f"k{k}_end" not in want[2 * k][0] for k in range(len(tails))) and all(x != "DEPTH" for x in want)
    return rels, queries, want


@pytest.mark.parametrize("world", [2, 3])
def test_least_level_through_inlined_userset(aclgpu, least_level_case, world):
    """doc and group sit on different shards: the marks of one lookup's states are decided on the owner, in the iteration before their level --
    the test that fails when a visit is decided in the wrong iteration (a state would count one level too deep and `end` would drop out)."""
    rels, queries, want = least_level_case

    def run(se):
        return [answer(aclgpu, se, rt, rid, perm, st, srel, want_excluded=False) for rt, rid, perm, st, srel in queries]

    for got in run_shards(aclgpu, world, SCHEMA_CHAIN, lambda e: e.touch(*rels), run):
        for q, g, wnt in zip(queries, got, want):
            assert g == wnt, (world, q)


# ---------------------------------------------------------------------------------------------------------------- 5: wildcards and combine schemas
WILD_DOCS = ["d1", "d2", "d3", "d4", "d5", "d6", "d7", "d8", "nobody"]
WILD_PERMS = ["view", "both", "allp", "mixed", "open"]


@pytest.fixture(scope="module")
def wild_want():
    names = names_of(WILD_RELS, "user")
    return {lenient: {(d, p): contract(SCHEMA_WILD, WILD_RELS, "doc", d, p, "user", "", names, lenient=lenient) for d in WILD_DOCS for p in WILD_PERMS}
            for lenient in (False, True)}


@pytest.mark.parametrize("lenient", [False, True])
def test_wildcards_and_combine_schemas(aclgpu, wild_want, lenient):
    """World 8 (doc 2, group 1, folder 6): candidates by the positive relaxation, confirmed by ONE sharded Check every shard takes part in; the
    wildcard's stand-in and the excluded rows the same way."""
    want = wild_want[lenient]

    def load(e):
        e.touch(*WILD_RELS)
        e.intern("doc", "nobody")

    def run(se):
        return {(d, p): answer(aclgpu, se, "doc", d, p, "user") for d in WILD_DOCS for p in WILD_PERMS}

    outs = run_shards(aclgpu, 8, SCHEMA_WILD, load, run, lenient_lookup=lenient)
    assert len(outs) == 8
    for got in outs:
        seen_wild = seen_ex = 0
        for key, wnt in want.items():
            assert got[key] == wnt, key
            if wnt != "DEPTH" and wnt[1]:
                seen_wild += 1
                seen_ex += bool(wnt[2])
        assert seen_wild >= 3 and seen_ex >= 1
        assert got[("d1", "view")][1] and got[("d1", "view")][2] == {"u1", "u2"}


def test_depth_failure_under_exclusion(aclgpu):
    """A subtracted branch beyond the limit: the reached subject's Check errs -- strict: ACL_ERR_DEPTH on EVERY rank; lenient: it is left out."""
    chain = [("group", f"c{i}", "member", "group", f"c{i + 1}", "member") for i in range(MAX_DEPTH + 2)]
    rels = [("doc", "d", "viewer", "user", "u9", ""), ("doc", "d", "viewer", "user", "u8", ""), ("doc", "d", "banned", "group", "c0", "member")] + chain
    rels += [("doc", "ok", "viewer", "user", "u9", ""), ("doc", "ok", "banned", "user", "u1", ""), ("doc", "far", "a", "group", "c0", "member"),
             ("group", f"c{MAX_DEPTH + 2}", "member", "user", "deep", ""), ("doc", "far", "viewer", "user", "u9", "")]
    names = names_of(rels, "user")
    queries = [("d", "view"), ("ok", "view"), ("far", "mixed"), ("far", "both")]
    for lenient in (False, True):
        want = [contract(SCHEMA_WILD, rels, "doc", d, p, "user", "", names, lenient=lenient) for d, p in queries]
        assert (want[0] == "DEPTH") != lenient and want[1][0] == {"u9"}
        if lenient:
            assert want[0][0] == set()

        def run(se):
            return [answer(aclgpu, se, "doc", d, p, "user") for d, p in queries]

        outs = run_shards(aclgpu, 8, SCHEMA_WILD, lambda e: e.touch(*rels), run, lenient_lookup=lenient)
        assert len(outs) == 8
        for got in outs:
            assert got == want, lenient

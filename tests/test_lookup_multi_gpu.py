"""LookupResources against many (type, permission) targets in ONE reverse walk per subject (acl_lookup_resources_multi, k_rev_multi) on the GPU.
Every row must equal lookup_ids_batch of its target alone AND the oracles' id sets (oracle.orc everywhere, oracle.pyoracle on the hand graphs); the new
kernel must really be the one that ran (stats), `visited` must come back all zero, and every fallback must give the same rows."""
import ctypes as C

import numpy as np
import pytest

from oracle import orc
from oracle.pyoracle import PyOracle

pytestmark = pytest.mark.gpu

C4_TARGETS = [("group", "member"), ("namespace", "viewer"), ("namespace", "creator"), ("namespace", "view"),
              ("pod", "namespace"), ("pod", "viewer"), ("pod", "creator"), ("pod", "view")]


@pytest.fixture(scope="module")
def aclgpu(aclgpu_lib):
    import aclgpu as m
    return m


def ids_of(row):
    return np.flatnonzero(np.unpackbits(np.ascontiguousarray(row).view(np.uint8), bitorder="little")).astype(np.uint32)


def names_of(e, rt, row):
    return {e.object_name(rt, int(i)) for i in ids_of(row)}


def multi_vs_single(e, targets, stype, srel, sids):
    """the multi call's rows; each compared bit for bit with lookup_ids_batch of its target alone, counts with popcounts"""
    rows, counts = e.lookup_ids_multi(targets, stype, srel, sids)
    assert len(rows) == len(targets) and counts.shape == (len(sids), len(targets))
    for j, (rt, pm) in enumerate(targets):
        b1, c1 = e.lookup_ids_batch(rt, pm, stype, srel, sids)
        assert np.array_equal(rows[j], b1), (rt, pm)
        assert np.array_equal(counts[:, j], c1), (rt, pm)
        assert [int(c) for c in counts[:, j]] == [ids_of(r).size for r in rows[j]], (rt, pm)
    return rows, counts


def hand_graph():
    """C4's schema: three users, groups nested three deep (and one group#member subject), two namespaces, six pods"""
    rels = [("group", "g1", "member", "user", "ann", ""), ("group", "g2", "member", "group", "g1", "member"), ("group", "g3", "member", "group", "g2", "member"),
            ("group", "g3", "member", "user", "bob", ""), ("group", "side", "member", "user", "cy", ""),
            ("namespace", "n1", "viewer", "group", "g3", "member"), ("namespace", "n1", "creator", "user", "cy", ""), ("namespace", "n2", "viewer", "user", "ann", ""),
            ("namespace", "n2", "creator", "user", "bob", "")]
    for p in range(6):
        rels.append(("pod", f"p{p}", "namespace", "namespace", "n1" if p < 4 else "n2", ""))
    rels += [("pod", "p0", "viewer", "user", "ann", ""), ("pod", "p4", "viewer", "group", "g2", "member"), ("pod", "p5", "viewer", "group", "side", "member"),
             ("pod", "p1", "creator", "user", "bob", ""), ("pod", "p5", "creator", "user", "ann", ""), ("pod", "p2", "viewer", "user", "cy", "")]
    return rels


def test_hand_graph_all_slots_pairs_and_a_userset_subject(aclgpu):
    """a sink that stops being one (namespace#view beside pod#view), a marked-through relation that is itself asked for (pod#viewer beside pod#view), NOMARK seed
    slots as targets (the relations a user is named on), a non-sink target (group#member), and the reflexive seed of a group#member subject"""
    from aclgpu import workloads
    schema, rels = workloads.SCHEMA_C4, hand_graph()
    co, po = orc.Oracle(schema), PyOracle(schema)
    co.write([(orc.OP_TOUCH, r) for r in rels])
    for r in rels:
        po.touch(*r)
    with aclgpu.Engine(schema) as e:
        e.write([(aclgpu.OP_TOUCH, r) for r in rels])
        all9 = C4_TARGETS + [("pod", "view")]  # (every slot of the schema -- `user` has none -- and one of them twice: nine targets, nine rows)
        subjects = [("user", "", ["ann", "bob", "cy", "nobody"]), ("group", "member", ["g1", "g2", "side"])]
        for stype, srel, names in subjects:
            sids = [e.intern(stype, n) for n in names]
            for targets in (C4_TARGETS, all9, [("namespace", "view"), ("pod", "view")], [("pod", "viewer"), ("pod", "view")]):
                e.stats_reset()
                rows, _counts = e.lookup_ids_multi(targets, stype, srel, sids)
                assert e.stats()["rev_multi_passes"] == 1 and e.stats()["rev_local_passes"] == 0 and e.stats()["expand_launches"] == 0
                multi_vs_single(e, targets, stype, srel, sids)
                for j, (rt, pm) in enumerate(targets):
                    for i, n in enumerate(names):
                        got = names_of(e, rt, rows[j][i])
                        assert got == co.lookup(rt, pm, stype, n, srel) == po.lookup_resources(rt, pm, stype, n, srel), (rt, pm, stype, n)
        ann = e.intern("user", "ann")
        rows, _ = e.lookup_ids_multi(C4_TARGETS, "user", "", [ann])
        assert names_of(e, "pod", rows[7][0]) == {"p0", "p1", "p2", "p3", "p4", "p5"} and names_of(e, "group", rows[0][0]) == {"g1", "g2", "g3"}


DEPTH_SCHEMA = """
definition user {}
definition group { relation member: user | group#member }
definition doc {
  relation viewer: user | group#member
  relation owner: user
  permission view = viewer + owner
}
"""


def test_depth_limit_each_target_keeps_its_own_rule(aclgpu):
    """doc#viewer and doc#view asked together: a doc whose viewer group sits K groups above the user is in `viewer` iff K + 1 <= 50 and in `view` iff K + 2 <= 50
    (the graph of test_relation_that_only_feeds_the_result_permission_is_marked_through_exactly); group#member holds 50 of the 55 groups"""
    rels = [("group", "g1", "member", "user", "deep", "")] + [("group", f"g{i + 1}", "member", "group", f"g{i}", "member") for i in range(1, 55)]
    rels += [("doc", f"d{k}", "viewer", "group", f"g{k}", "member") for k in range(40, 56)] + [("doc", "direct", "viewer", "user", "deep", ""), ("doc", "own", "owner", "user", "deep", "")]
    o = orc.Oracle(DEPTH_SCHEMA)
    o.write([(orc.OP_TOUCH, r) for r in rels])
    want = {("doc", "view"): {f"d{k}" for k in range(40, 49)} | {"direct", "own"}, ("doc", "viewer"): {f"d{k}" for k in range(40, 50)} | {"direct"},
            ("group", "member"): {f"g{k}" for k in range(1, 51)}}
    for t, w in want.items():
        assert o.lookup(t[0], t[1], "user", "deep") == w, t
    with aclgpu.Engine(DEPTH_SCHEMA) as e:
        e.write([(aclgpu.OP_TOUCH, r) for r in rels])
        deep = e.intern("user", "deep")
        for targets in ([("doc", "viewer"), ("doc", "view"), ("group", "member")], [("group", "member"), ("doc", "view"), ("doc", "viewer")]):
            e.stats_reset()
            rows, counts = e.lookup_ids_multi(targets, "user", "", [deep])
            assert e.stats()["rev_multi_passes"] == 1
            for j, t in enumerate(targets):
                assert names_of(e, t[0], rows[j][0]) == want[t], t
                assert counts[0, j] == len(want[t])
            multi_vs_single(e, targets, "user", "", [deep])


def test_cycles_and_wildcards(aclgpu):
    schema = "definition user {}\ndefinition group { relation member: user | group#member }\ndefinition doc { relation viewer: user | user:* | group#member\n relation owner: user\n permission view = viewer + owner }"
    rels = [("group", "c0", "member", "group", "c1", "member"), ("group", "c1", "member", "group", "c2", "member"), ("group", "c2", "member", "group", "c0", "member"),
            ("group", "c1", "member", "user", "loop", ""), ("doc", "open", "viewer", "user", "*", ""), ("doc", "mine", "owner", "user", "loop", ""),
            ("doc", "team", "viewer", "group", "c0", "member")]
    co, po = orc.Oracle(schema), PyOracle(schema)
    co.write([(orc.OP_TOUCH, r) for r in rels])
    for r in rels:
        po.touch(*r)
    targets = [("group", "member"), ("doc", "viewer"), ("doc", "owner"), ("doc", "view")]
    with aclgpu.Engine(schema) as e:
        e.write([(aclgpu.OP_TOUCH, r) for r in rels])
        names = ["loop", "stranger"]  # (`stranger` holds no relationship: only the wildcard reaches it)
        sids = [e.intern("user", n) for n in names]
        e.stats_reset()
        rows, _ = multi_vs_single(e, targets, "user", "", sids)
        assert e.stats()["rev_multi_passes"] == 1
        for j, (rt, pm) in enumerate(targets):
            for i, n in enumerate(names):
                assert names_of(e, rt, rows[j][i]) == co.lookup(rt, pm, "user", n) == po.lookup_resources(rt, pm, "user", n), (rt, pm, n)
        assert names_of(e, "group", rows[0][0]) == {"c0", "c1", "c2"} and names_of(e, "doc", rows[3][1]) == {"open"}
        gs = [e.intern("group", "c2")]
        rows, _ = multi_vs_single(e, targets, "group", "member", gs)
        for j, (rt, pm) in enumerate(targets):
            assert names_of(e, rt, rows[j][0]) == co.lookup(rt, pm, "group", "c2", "member"), (rt, pm)


NONMONO_SCHEMA = """
definition user {}
definition g { relation member: user | g#member }
definition folder {
  relation viewer: user | g#member
  relation banned: user | g#member
  permission view = viewer - banned
}
definition doc {
  relation parent: folder
  relation viewer: user | g#member
  relation owner: user | g#member
  relation banned: user | g#member
  permission view = viewer - banned
  permission both = viewer & owner
  permission every = parent.all(view)
}
"""


def test_non_monotone_targets_mixed_with_monotone_ones(aclgpu):
    """`-`, `&` and `.all()` targets beside plain relations in one call: candidates are confirmed per target; a candidate whose Check ends at the depth
    limit fails the call with ACL_ERR_DEPTH, and under ACL_FLAG_LENIENT_LOOKUP it is left out -- as the single-target call does for that target"""
    rels = [("g", "g0", "member", "user", "deep", "")] + [("g", f"g{i + 1}", "member", "g", f"g{i}", "member") for i in range(60)]
    rels += [("folder", "f1", "viewer", "user", "u", ""), ("folder", "f2", "viewer", "user", "u", ""), ("folder", "f2", "banned", "user", "u", ""), ("folder", "f3", "viewer", "user", "v", ""),
             ("doc", "x", "viewer", "user", "u", ""), ("doc", "x", "owner", "user", "u", ""), ("doc", "y", "viewer", "user", "u", ""), ("doc", "y", "banned", "user", "u", ""),
             ("doc", "z", "owner", "user", "u", ""), ("doc", "z", "viewer", "user", "v", ""), ("doc", "x", "parent", "folder", "f1", ""), ("doc", "y", "parent", "folder", "f1", ""),
             ("doc", "y", "parent", "folder", "f2", ""), ("doc", "z", "parent", "folder", "f3", ""), ("doc", "w", "viewer", "g", "g3", "member"), ("doc", "w", "owner", "user", "deep", "")]
    tainted = [("doc", "e1", "viewer", "user", "deep", ""), ("doc", "e1", "banned", "g", "g59", "member")]  # e1 is a candidate of `deep` whose Check errs
    targets = [("doc", "view"), ("doc", "viewer"), ("doc", "both"), ("folder", "view"), ("doc", "every"), ("g", "member")]
    co, po = orc.Oracle(NONMONO_SCHEMA), PyOracle(NONMONO_SCHEMA)
    co.write([(orc.OP_TOUCH, r) for r in rels])
    for r in rels:
        po.touch(*r)
    names = ["u", "v", "deep"]
    with aclgpu.Engine(NONMONO_SCHEMA) as e:
        e.write([(aclgpu.OP_TOUCH, r) for r in rels])
        sids = [e.intern("user", n) for n in names]
        e.stats_reset()
        rows, _ = multi_vs_single(e, targets, "user", "", sids)
        assert e.stats()["rev_multi_passes"] == 1
        for j, (rt, pm) in enumerate(targets):
            for i, n in enumerate(names):
                assert names_of(e, rt, rows[j][i]) == co.lookup(rt, pm, "user", n) == po.lookup_resources(rt, pm, "user", n), (rt, pm, n)
        assert names_of(e, "doc", rows[0][0]) == {"x"} and names_of(e, "doc", rows[2][0]) == {"x"} and names_of(e, "doc", rows[4][0]) == {"x"}
        e.write([(aclgpu.OP_TOUCH, r) for r in tainted])
        with pytest.raises(aclgpu.AclError) as ei:
            e.lookup_ids_multi(targets, "user", "", sids)
        assert ei.value.code == aclgpu.ERR_DEPTH and "max depth exceeded" in str(ei.value)
        with pytest.raises(aclgpu.AclError) as ei:  # (the single-target call fails the same way)
            e.lookup_ids_batch("doc", "view", "user", "", sids)
        assert ei.value.code == aclgpu.ERR_DEPTH
        ok, _ = e.lookup_ids_multi([("doc", "viewer"), ("g", "member")], "user", "", sids)  # (monotone targets alone still answer)
        assert "e1" in names_of(e, "doc", ok[0][2])
    co.write([(orc.OP_TOUCH, r) for r in tainted])
    co.set_lenient_lookup(True)
    with aclgpu.Engine(NONMONO_SCHEMA, lenient_lookup=True) as e:
        e.write([(aclgpu.OP_TOUCH, r) for r in rels + tainted])
        sids = [e.intern("user", n) for n in names]
        rows, _ = multi_vs_single(e, targets, "user", "", sids)
        for j, (rt, pm) in enumerate(targets):
            for i, n in enumerate(names):
                assert names_of(e, rt, rows[j][i]) == co.lookup(rt, pm, "user", n), (rt, pm, n)
        assert "e1" not in names_of(e, "doc", rows[0][2]) and "e1" in names_of(e, "doc", rows[1][2])


@pytest.fixture(scope="module")
def c4_small():
    from aclgpu import workloads
    w = workloads.c4(scale=0.02, batch=1000, n_user=5000)
    o = orc.Oracle(w.schema)
    w.load(o)
    o.freeze()
    rng = np.random.default_rng(11)
    users = rng.integers(0, w.nobjects["user"], size=40).astype(np.uint32)
    groups = rng.integers(0, w.nobjects["group"], size=24).astype(np.uint32)
    return w, o, users, groups


def test_batch_equals_single_target_batches_and_the_oracle(aclgpu, c4_small):
    w, o, users, groups = c4_small
    targets = C4_TARGETS + [("pod", "view")]  # nine targets
    with aclgpu.Engine(w.schema) as e:
        w.load(e)
        e.stats_reset()
        got = {"user": e.lookup_ids_multi(targets, "user", "", users), "group": e.lookup_ids_multi(targets, "group", "member", groups)}
        st = e.stats()
        assert st["rev_multi_passes"] == 2 and st["rev_local_passes"] == 0 and st["expand_launches"] == 0 and st["lookup_requests"] == 64 * 9
        def oracle_ids(rt, pm, stype, srel, sid):
            """LookupResources by the oracle = the resources its Check grants; over the 16 900 pods the per-resource Checks are spread over
            16 host threads (orc.lookup_ids runs the same Checks on one: 0.5-0.8 s per pod lookup), the small types go through lookup_ids itself"""
            if rt != "pod":
                return np.sort(o.lookup_ids(rt, pm, stype, srel, sid))
            n = w.nobjects[rt]
            perm, err = o.check_bulk_ids_mt(16, rt, pm, np.arange(n, dtype=np.uint32), stype, srel, np.full(n, sid, dtype=np.uint32))
            assert not err.any()
            return np.flatnonzero(perm == 2).astype(np.uint32)

        assert np.array_equal(oracle_ids("pod", "view", "user", "", int(users[0])), np.sort(o.lookup_ids("pod", "view", "user", "", int(users[0]))))  # (the two forms agree)
        for stype, (rows, counts) in got.items():
            subs, srel = (users, "") if stype == "user" else (groups, "member")
            for j, (rt, pm) in enumerate(targets):
                if targets.index((rt, pm)) < j:  # (the duplicate target: its own row, equal to the first one's -- compared once)
                    assert np.array_equal(rows[j], rows[targets.index((rt, pm))]) and np.array_equal(counts[:, j], counts[:, targets.index((rt, pm))])
                    continue
                b1, c1 = e.lookup_ids_batch(rt, pm, stype, srel, subs)
                assert np.array_equal(rows[j], b1) and np.array_equal(counts[:, j], c1), (stype, rt, pm)
                for i in range(0, subs.size, 5):
                    want = oracle_ids(rt, pm, stype, srel, int(subs[i]))
                    assert np.array_equal(ids_of(rows[j][i]), want) and counts[i, j] == want.size, (stype, rt, pm, int(subs[i]))
        assert int(got["user"][1].max()) > 50  # (the graph is not degenerate)


def test_visited_is_handed_back_all_zero(aclgpu, c4_small):
    """multi, singles, multi, singles on ONE engine (one context: the same `visited` rows): a stale mark of either kernel would add ids to the other's rows"""
    w, _o, users, _groups = c4_small
    targets = C4_TARGETS
    singles = [("pod", "view"), ("group", "member"), ("namespace", "viewer")]
    with aclgpu.Engine(w.schema, contexts=1) as e:
        w.load(e)
        first = e.lookup_ids_multi(targets, "user", "", users)
        s1 = [e.lookup_ids_batch(rt, pm, "user", "", users) for rt, pm in singles]
        second = e.lookup_ids_multi(targets, "user", "", users)
        s2 = [e.lookup_ids_batch(rt, pm, "user", "", users) for rt, pm in singles]
        assert all(np.array_equal(a, b) for a, b in zip(first[0], second[0])) and np.array_equal(first[1], second[1])
        for (rt, pm), (b1, c1), (b2, c2) in zip(singles, s1, s2):
            j = targets.index((rt, pm))
            assert np.array_equal(b1, b2) and np.array_equal(c1, c2) and np.array_equal(b1, first[0][j]) and np.array_equal(c1, first[1][:, j]), (rt, pm)


def test_fallbacks_give_the_same_rows(aclgpu, c4_small, monkeypatch):
    w, _o, users, _groups = c4_small
    with aclgpu.Engine(w.schema) as e:
        w.load(e)
        want = e.lookup_ids_multi(C4_TARGETS, "user", "", users)
    monkeypatch.setenv("ACL_REV_LOCAL", "0")  # (read at acl_open): neither single-launch kernel -- target by target on the level loop
    with aclgpu.Engine(w.schema) as e:
        w.load(e)
        e.stats_reset()
        rows, counts = e.lookup_ids_multi(C4_TARGETS, "user", "", users)
        st = e.stats()
        assert st["rev_multi_passes"] == 0 and st["rev_local_passes"] == 0 and st["expand_launches"] > 0 and st["lookup_requests"] == users.size * len(C4_TARGETS)
        assert all(np.array_equal(a, b) for a, b in zip(rows, want[0])) and np.array_equal(counts, want[1])
    monkeypatch.delenv("ACL_REV_LOCAL")
    # a block that outgrows its log (the overflowing user of test_block_that_outgrows_its_region_falls_back): the group is answered target by target
    from aclgpu import workloads
    w3 = workloads.c3(scale=0.2, batch=256, power_users=8)
    big, nns = 7, w3.nobjects["namespace"]
    w3.edges.append(("namespace", "viewer", "user", "", np.arange(nns, dtype=np.uint32), np.full(nns, big, dtype=np.uint32)))
    w3.edges.append(("pod", "viewer", "user", "", np.arange(100, 800, dtype=np.uint32), np.full(700, big, dtype=np.uint32)))
    o3 = orc.Oracle(w3.schema)
    w3.load(o3)
    o3.freeze()
    targets = [("namespace", "view"), ("pod", "view")]
    subs = np.concatenate([w3.lookup_subjects[:4], np.asarray([big], dtype=np.uint32)])
    monkeypatch.setenv("ACL_LOCAL_CAP", "256")
    with aclgpu.Engine(w3.schema) as e:
        w3.load(e)
        e.stats_reset()
        rows, counts = e.lookup_ids_multi(targets, "user", "", subs)
        st = e.stats()
        assert st["overflow_retries"] >= 1 and st["rev_multi_passes"] == 0
        for j, (rt, pm) in enumerate(targets):
            for i, s in enumerate(subs):
                wid = np.sort(o3.lookup_ids(rt, pm, "user", "", int(s)))
                assert np.array_equal(ids_of(rows[j][i]), wid) and counts[i, j] == wid.size, (rt, pm, int(s))
        assert counts[-1, 1] >= 700
        e.stats_reset()
        r4, c4 = e.lookup_ids_multi(targets, "user", "", subs[:4])  # the others fit: the one walk answers
        assert e.stats()["rev_multi_passes"] == 1 and e.stats()["overflow_retries"] == 0
        assert all(np.array_equal(a, b[:4]) for a, b in zip(r4, rows)) and np.array_equal(c4, counts[:4])


def test_callers_buffers_duplicates_and_access_review(aclgpu):
    from aclgpu import workloads
    from aclgpu._lib import Target
    schema, rels = workloads.SCHEMA_C4, hand_graph()
    with aclgpu.Engine(schema) as e:
        e.write([(aclgpu.OP_TOUCH, r) for r in rels])
        sids = np.asarray([e.intern("user", n) for n in ("ann", "bob", "cy")], dtype=np.uint32)
        targets = [("pod", "view"), ("group", "member"), ("pod", "view")]
        rows, counts = e.lookup_ids_multi(targets, "user", "", sids)
        assert np.array_equal(rows[0], rows[2]) and np.array_equal(counts[:, 0], counts[:, 2]) and rows[0].any()  # duplicate targets: identical rows of their own
        # more targets than the kernel stages in LDS (256): the descriptors behind them are read where they lie
        many, mc = e.lookup_ids_multi([("pod", "view"), ("group", "member")] * 150, "user", "", sids)
        for j in range(300):
            assert np.array_equal(many[j], rows[j % 2]) and np.array_equal(mc[:, j], counts[:, j % 2]), j
        need = [rows[j].shape[1] for j in range(3)]
        tg = (Target * 3)(*[Target(e.type_id(rt), e.relation_id(rt, pm)) for rt, pm in targets])

        def call(words, fill=0xFFFFFFFF):
            buf = np.full((sids.size, int(sum(words))), fill, dtype=np.uint32)
            cnt = np.zeros((sids.size, 3), dtype=np.uint64)
            ww = np.asarray(words, dtype=np.uintp)
            rc = e._L.acl_lookup_resources_multi(e._h, tg, 3, e.type_id("user"), -1, sids.ctypes.data, sids.size, buf.ctypes.data, ww.ctypes.data, cnt.ctypes.data, None)
            return rc, buf, cnt
        # rows wider than the types need: the tail words are zero
        wide = [need[0] + 7, need[1] + 3, need[2]]
        rc, buf, cnt = call(wide)
        assert rc == 0 and np.array_equal(cnt, counts)
        off = 0
        for j in range(3):
            assert np.array_equal(buf[:, off:off + need[j]], rows[j]) and not buf[:, off + need[j]:off + wide[j]].any(), j
            off += wide[j]
        # one word too narrow: refused, nothing written
        rc, buf, cnt = call([need[0], need[1] - 1, need[2]])
        assert rc == aclgpu.ERR_INVALID_ARGUMENT and (buf == 0xFFFFFFFF).all() and not cnt.any()
        # the audit form: one entry per slot of the schema, each equal to lookup()
        rev = e.access_review("user", "ann")
        assert sorted(rev) == sorted(C4_TARGETS) and len(rev) == 8
        for (rt, pm), got in rev.items():
            assert got == e.lookup(rt, pm, "user", "ann"), (rt, pm)
        assert rev[("pod", "view")] == {"p0", "p1", "p2", "p3", "p4", "p5"}
        part = e.access_review("group", "g1", "member", targets=[("namespace", "view"), ("group", "member")])
        assert part == {("namespace", "view"): e.lookup("namespace", "view", "group", "g1", "member"), ("group", "member"): e.lookup("group", "member", "group", "g1", "member")}
        assert e.access_review("user", "never-seen") == {t: set() for t in C4_TARGETS}

"""LookupSubjects on the GPU (k_subj_local + engine_subjects.cpp) against the oracles' Check.

The contract: ids = {s : Relaxed'(s) == HAS and Check(s) == HAS}, where Relaxed' is the Check under the positive relaxation of the schema
(`a - b` -> a, `a & b` -> a + b, `a.all(b)` -> a->b) on the relationships minus the `T:*` ones; wildcard = Relaxed(fresh) == HAS and
Check(fresh) == HAS for a subject nobody names; excluded = {s : Check(s) != HAS} when wildcard; a reached subject whose Check errs fails
the call with ACL_ERR_DEPTH (ACL_FLAG_LENIENT_LOOKUP: it is left out)."""
import numpy as np
import pytest

from oracle import orc
from oracle.pyoracle import MAX_DEPTH
from tests.subjects_contract import contract

pytestmark = pytest.mark.gpu

PERM_HAS = 2


@pytest.fixture(scope="module")
def aclgpu(aclgpu_lib):
    import aclgpu as m
    return m


def ids_of(row):
    return set(np.flatnonzero(np.unpackbits(np.ascontiguousarray(row, dtype=np.uint32).view(np.uint8), bitorder="little")).tolist())


def subjects_of_type(e, st):
    """every name of the subject type the engine holds but the wildcard's own"""
    return [n for n in (e.object_name(st, i) for i in range(e.object_count(st))) if n != "*"]


def engine_answer(aclgpu, e, rt, rid, perm, st, srel=""):
    try:
        return e.lookup_subjects(rt, rid, perm, st, srel)
    except aclgpu.AclError as x:
        if x.code == aclgpu.ERR_DEPTH:
            return "DEPTH"
        raise


def check_rows(o, rt, perm, rids, st, srel, nobj):
    """expected rows by the C oracle's Check over R x U (monotone permissions: ids = {s : Check == HAS})"""
    out = []
    subj = np.arange(nobj, dtype=np.uint32)
    for r in rids:
        p, _ = o.check_bulk_ids_mt(8, rt, perm, np.full(nobj, r, dtype=np.uint32), st, srel, subj)
        out.append(set(np.flatnonzero(p == PERM_HAS).tolist()))
    return out


@pytest.mark.parametrize("cfg", ["c3", "c4"])
def test_workload_parity(aclgpu, cfg):
    """C3 and C4 at a small scale, ~64 pods (one with no relationships): the batched rows and the one-by-one rows equal {s : Check == HAS}."""
    from aclgpu import workloads
    w = workloads.c3(scale=0.01) if cfg == "c3" else workloads.c4(scale=0.01, n_user=2000)
    o = orc.Oracle(w.schema)
    w.load(o)
    with aclgpu.Engine(w.schema, device=0) as e:
        w.load(e)
        npod = e.object_count("pod")
        rids = np.unique(np.concatenate([np.random.default_rng(11).choice(npod, size=63, replace=False), [0]]).astype(np.uint32))
        empty = e.intern("pod", "no-relationships-at-all")
        rids = np.append(rids, np.uint32(empty))
        o.intern("pod", "no-relationships-at-all")
        nuser = e.object_count("user")
        bms, counts, flags = e.lookup_subjects_ids_batch("pod", "view", "user", "", rids)
        want = check_rows(o, "pod", "view", rids, "user", "", nuser)
        for i, r in enumerate(rids):
            assert ids_of(bms[i]) == want[i], (cfg, int(r))
            assert int(counts[i]) == len(want[i]) and flags[i] == 0
        assert not want[-1]
        assert sum(len(x) for x in want) > 0
        for i in range(0, len(rids), 7):  # n = 1 equals the batched form
            b1, c1, _ = e.lookup_subjects_ids_batch("pod", "view", "user", "", rids[i:i + 1])
            assert np.array_equal(b1[0], bms[i]) and c1[0] == counts[i]


def test_subject_relation(aclgpu):
    """LookupSubjects(pod, view, group, member) against the Check over all groups, and the reflexive (group, member, group, member)."""
    from aclgpu import workloads
    w = workloads.c4(scale=0.005, n_user=500)
    o = orc.Oracle(w.schema)
    w.load(o)
    with aclgpu.Engine(w.schema, device=0) as e:
        w.load(e)
        ngroup = e.object_count("group")
        rids = np.random.default_rng(3).choice(e.object_count("pod"), size=32, replace=False).astype(np.uint32)
        bms, counts, _ = e.lookup_subjects_ids_batch("pod", "view", "group", "member", rids)
        want = check_rows(o, "pod", "view", rids, "group", "member", ngroup)
        assert sum(len(x) for x in want) > 0
        for i in range(len(rids)):
            assert ids_of(bms[i]) == want[i]
        gids = np.arange(0, ngroup, max(1, ngroup // 24), dtype=np.uint32)
        bms, _, _ = e.lookup_subjects_ids_batch("group", "member", "group", "member", gids)
        want = check_rows(o, "group", "member", gids, "group", "member", ngroup)
        for i, g in enumerate(gids):
            assert int(g) in want[i] and ids_of(bms[i]) == want[i]


SCHEMA_CHAIN = """
definition user {}
definition group {
  relation member: user | group#member
}
definition doc {
  relation viewer: user | group#member
  relation editor: group#member
  permission edit = editor
  permission view = viewer + edit
  permission deep = d1
  permission d1 = d2
  permission d2 = d3
  permission d3 = d4
  permission d4 = viewer
}
"""


def _answer_vs_contract(aclgpu, e, schema, rels, rt, rid, perm, st, srel="", lenient=False, now=0):
    names = subjects_of_type(e, st)
    want = contract(schema, rels, rt, rid, perm, st, srel, names, lenient=lenient, now=now)
    got = engine_answer(aclgpu, e, rt, rid, perm, st, srel)
    assert got == want, (rt, rid, perm, st, srel)
    return got


def test_depth_limit_chains(aclgpu):
    """Userset chains ending just inside, at and beyond the dispatch-depth limit: the end subject is listed or silently out, as Check says."""
    for length in range(MAX_DEPTH - 6, MAX_DEPTH + 2):
        rels = [("doc", "d", "viewer", "group", "g0", "member")]
        rels += [("group", f"g{i}", "member", "group", f"g{i + 1}", "member") for i in range(length)]
        rels += [("group", f"g{i}", "member", "user", f"u{i}", "") for i in range(0, length + 1)]
        with aclgpu.Engine(SCHEMA_CHAIN, device=0) as e:
            e.touch(*rels)
            got = _answer_vs_contract(aclgpu, e, SCHEMA_CHAIN, rels, "doc", "d", "view", "user")
            assert got != "DEPTH" and "u0" in got[0] and (f"u{length}" in got[0]) == (length <= MAX_DEPTH - 3)
            _answer_vs_contract(aclgpu, e, SCHEMA_CHAIN, rels, "doc", "d", "deep", "user")
            _answer_vs_contract(aclgpu, e, SCHEMA_CHAIN, rels, "doc", "d", "view", "group", "member")


def test_depth_short_path_through_inlined_userset(aclgpu):
    """One group reached by a long path (a chain of groups the walk enumerates first) and by a short one (an inlined computed userset):
    the subjects below it count from the short path's level."""
    for tail in range(MAX_DEPTH - 8, MAX_DEPTH - 1):
        rels = [("doc", "d", "viewer", "group", "a0", "member")]
        rels += [("group", f"a{i}", "member", "group", f"a{i + 1}", "member") for i in range(6)]
        rels += [("group", "a6", "member", "group", "x", "member"), ("doc", "d", "editor", "group", "x", "member")]
        rels += [("group", "x", "member", "group", "t0", "member")]
        rels += [("group", f"t{i}", "member", "group", f"t{i + 1}", "member") for i in range(tail)]
        rels += [("group", f"t{tail}", "member", "user", "end", "")]
        with aclgpu.Engine(SCHEMA_CHAIN, device=0) as e:
            e.touch(*rels)
            _answer_vs_contract(aclgpu, e, SCHEMA_CHAIN, rels, "doc", "d", "view", "user")
            _answer_vs_contract(aclgpu, e, SCHEMA_CHAIN, rels, "doc", "d", "deep", "user")
    # the end subject must be in at least one of these (the short path reaches it within the limit, the long one does not)
    rels = [("doc", "d", "viewer", "group", "a0", "member")]
    rels += [("group", f"a{i}", "member", "group", f"a{i + 1}", "member") for i in range(6)]
    rels += [("group", "a6", "member", "group", "x", "member"), ("doc", "d", "editor", "group", "x", "member"), ("group", "x", "member", "group", "t0", "member")]
    tail = MAX_DEPTH - 6
    rels += [("group", f"t{i}", "member", "group", f"t{i + 1}", "member") for i in range(tail)] + [("group", f"t{tail}", "member", "user", "end", "")]
    with aclgpu.Engine(SCHEMA_CHAIN, device=0) as e:
        e.touch(*rels)
        got = _answer_vs_contract(aclgpu, e, SCHEMA_CHAIN, rels, "doc", "d", "view", "user")
        assert "end" in got[0]


def test_group_cycle_below_a_pod(aclgpu):
    rels = [("doc", "d", "viewer", "group", "g0", "member"), ("group", "g0", "member", "group", "g1", "member"),
            ("group", "g1", "member", "group", "g2", "member"), ("group", "g2", "member", "group", "g0", "member"),
            ("group", "g0", "member", "user", "alice", ""), ("group", "g2", "member", "user", "bob", ""), ("doc", "d", "viewer", "user", "carol", "")]
    with aclgpu.Engine(SCHEMA_CHAIN, device=0) as e:
        e.touch(*rels)
        got = _answer_vs_contract(aclgpu, e, SCHEMA_CHAIN, rels, "doc", "d", "view", "user")
        assert got[0] == {"alice", "bob", "carol"}
        _answer_vs_contract(aclgpu, e, SCHEMA_CHAIN, rels, "group", "g1", "member", "group", "member")


SCHEMA_WILD = """
definition user {}
definition group {
  relation member: user | group#member
}
definition folder {
  relation viewer: user | user:* | group#member
  permission see = viewer
}
definition doc {
  relation viewer: user | user:* | group#member
  relation banned: user | user:* | group#member
  relation a: user | group#member
  relation b: user | group#member
  relation parent: folder
  permission view = viewer - banned
  permission both = a & b
  permission allp = parent.all(see)
  permission mixed = (viewer + a) - (banned & b)
  permission open = viewer
}
"""

WILD_RELS = [
    ("doc", "d1", "viewer", "user", "*", ""), ("doc", "d1", "banned", "user", "u1", ""), ("doc", "d1", "banned", "group", "g1", "member"),
    ("group", "g1", "member", "user", "u2", ""),
    ("doc", "d2", "viewer", "user", "u1", ""), ("doc", "d2", "viewer", "user", "u2", ""), ("doc", "d2", "viewer", "user", "u3", ""),
    ("doc", "d2", "banned", "user", "u2", ""),
    ("doc", "d3", "viewer", "user", "*", ""), ("doc", "d3", "banned", "user", "*", ""), ("doc", "d3", "viewer", "user", "u4", ""),
    ("doc", "d4", "a", "user", "u1", ""), ("doc", "d4", "a", "user", "u2", ""), ("doc", "d4", "b", "user", "u2", ""), ("doc", "d4", "b", "group", "g1", "member"),
    ("doc", "d4", "a", "group", "g2", "member"), ("group", "g2", "member", "user", "u5", ""), ("doc", "d4", "b", "user", "u5", ""),
    ("doc", "d5", "parent", "folder", "f1", ""), ("doc", "d5", "parent", "folder", "f2", ""), ("folder", "f1", "viewer", "user", "u1", ""),
    ("folder", "f1", "viewer", "user", "u2", ""), ("folder", "f2", "viewer", "user", "u2", ""), ("folder", "f2", "viewer", "group", "g2", "member"),
    ("doc", "d6", "parent", "folder", "f3", ""), ("folder", "f3", "viewer", "user", "*", ""),
    ("doc", "d7", "viewer", "user", "u3", ""), ("doc", "d7", "a", "user", "u4", ""),
    ("doc", "d7", "banned", "user", "u4", ""), ("doc", "d7", "b", "user", "u4", ""), ("doc", "d7", "banned", "user", "u3", ""),
    ("doc", "d8", "viewer", "user", "*", ""), ("doc", "d8", "viewer", "user", "u6", ""),
]


@pytest.mark.parametrize("lenient", [False, True])
def test_wildcards_and_combine_schemas(aclgpu, lenient):
    with aclgpu.Engine(SCHEMA_WILD, device=0, lenient_lookup=lenient) as e:
        e.touch(*WILD_RELS)
        seen_wild = seen_ex = 0
        for d in ["d1", "d2", "d3", "d4", "d5", "d6", "d7", "d8", "nobody"]:
            for p in ["view", "both", "allp", "mixed", "open"]:
                got = _answer_vs_contract(aclgpu, e, SCHEMA_WILD, WILD_RELS, "doc", d, p, "user", lenient=lenient)
                if got != "DEPTH" and got[1]:
                    seen_wild += 1
                    seen_ex += bool(got[2])
            _answer_vs_contract(aclgpu, e, SCHEMA_WILD, WILD_RELS, "doc", d, "view", "group", "member", lenient=lenient)
        assert seen_wild >= 3 and seen_ex >= 1
        got = e.lookup_subjects("doc", "d1", "view", "user")
        assert got[1] and got[2] == {"u1", "u2"}


def test_depth_failure_under_exclusion(aclgpu):
    """A subtracted branch beyond the limit: the reached subject's Check errs -> ACL_ERR_DEPTH; lenient: it is left out."""
    chain = [("group", f"c{i}", "member", "group", f"c{i + 1}", "member") for i in range(MAX_DEPTH + 2)]
    rels = [("doc", "d", "viewer", "user", "u9", ""), ("doc", "d", "viewer", "user", "u8", ""), ("doc", "d", "banned", "group", "c0", "member")] + chain
    rels += [("doc", "ok", "viewer", "user", "u9", ""), ("doc", "ok", "banned", "user", "u1", ""), ("doc", "far", "a", "group", "c0", "member"),
             ("group", f"c{MAX_DEPTH + 2}", "member", "user", "deep", ""), ("doc", "far", "viewer", "user", "u9", "")]
    for lenient in (False, True):
        with aclgpu.Engine(SCHEMA_WILD, device=0, lenient_lookup=lenient) as e:
            e.touch(*rels)
            got = _answer_vs_contract(aclgpu, e, SCHEMA_WILD, rels, "doc", "d", "view", "user", lenient=lenient)
            assert (got == "DEPTH") != lenient
            if lenient:
                assert got[0] == set()
            assert _answer_vs_contract(aclgpu, e, SCHEMA_WILD, rels, "doc", "ok", "view", "user", lenient=lenient)[0] == {"u9"}
            _answer_vs_contract(aclgpu, e, SCHEMA_WILD, rels, "doc", "far", "mixed", "user", lenient=lenient)
            _answer_vs_contract(aclgpu, e, SCHEMA_WILD, rels, "doc", "far", "both", "user", lenient=lenient)


SCHEMA_LIVE = """
definition user {}
definition group {
  relation member: user | group#member
}
definition doc {
  relation viewer: user with expiration | group#member
  permission view = viewer
}
"""


def test_live_graph_and_replicas(aclgpu):
    """touch, delete and expiry between lookups follow the oracle; two logical replicas answer alike after a write."""
    rels = [("doc", "d", "viewer", "user", "u1", "", 0), ("doc", "d", "viewer", "group", "g", "member", 0), ("group", "g", "member", "user", "u2", "", 0),
            ("doc", "d", "viewer", "user", "u3", "", 100)]
    with aclgpu.Engine(SCHEMA_LIVE, devices=[0, 0]) as e:
        e.set_now(10)
        e.write([(aclgpu.OP_TOUCH, r[:6], r[6]) for r in rels])

        def expect(now):
            want = contract(SCHEMA_LIVE, rels, "doc", "d", "view", "user", "", subjects_of_type(e, "user"), now=now)
            for _ in range(4):  # (calls spread over both replicas)
                assert e.lookup_subjects("doc", "d", "view", "user") == want
            return want[0]

        assert expect(10) == {"u1", "u2", "u3"}
        e.touch(("group", "g", "member", "user", "u4", ""))
        rels.append(("group", "g", "member", "user", "u4", "", 0))
        assert expect(10) == {"u1", "u2", "u3", "u4"}
        e.delete_by_filter(rtype="doc", rid="d", rel="viewer", stype="user", sid="u1")
        rels = [r for r in rels if r[4] != "u1"]
        assert expect(10) == {"u2", "u3", "u4"}
        e.set_now(200)
        assert expect(200) == {"u2", "u4"}
        calls = dict()
        for dev, n in e.replica_calls():
            calls[dev] = calls.get(dev, 0) + n
        assert sum(calls.values()) > 0


SCHEMA_BIG = """
definition user {}
definition group {
  relation member: user | group#member
}
definition pod {
  relation viewer: user | group#member
  permission view = viewer
}
"""


def test_large_subject_space_and_region_overflow(aclgpu):
    """A subject type of more than 2^20 ids (the row leaves the LDS) and a pod viewed by 20 000 groups (the block's region overflows): both
    still equal the oracle's Check."""
    rng = np.random.default_rng(5)
    nuser = (1 << 20) + 70000
    o = orc.Oracle(SCHEMA_BIG)
    with aclgpu.Engine(SCHEMA_BIG, device=0) as e:
        pv_r = np.repeat(np.arange(8, dtype=np.uint32), 300)
        pv_s = rng.integers(0, nuser, size=pv_r.size).astype(np.uint32)
        pv_s[:8] = nuser - 1 - np.arange(8, dtype=np.uint32)
        key = np.unique(pv_r.astype(np.uint64) << np.uint64(32) | pv_s.astype(np.uint64))
        pv_r, pv_s = (key >> np.uint64(32)).astype(np.uint32), (key & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        ngroup = 20000
        pg_r = np.full(ngroup, 8, dtype=np.uint32)
        pg_s = np.arange(ngroup, dtype=np.uint32)
        gu_r = np.arange(ngroup, dtype=np.uint32)
        gu_s = rng.integers(0, nuser, size=ngroup).astype(np.uint32)
        gu_s[0] = nuser - 1
        for t in (e, o):
            t.add_edges("pod", "viewer", "user", "", pv_r, pv_s)
            t.add_edges("pod", "viewer", "group", "member", pg_r, pg_s)
            t.add_edges("group", "member", "user", "", gu_r, gu_s)
        assert e.object_count("user") > (1 << 20)
        rids = np.arange(9, dtype=np.uint32)
        bms, counts, _ = e.lookup_subjects_ids_batch("pod", "view", "user", "", rids)
        nu = e.object_count("user")
        want = check_rows(o, "pod", "view", rids[:8], "user", "", nu)  # (R x every user; the pods without groups are cheap for the oracle)
        for i in range(8):
            assert ids_of(bms[i]) == want[i], i
            assert int(counts[i]) == len(want[i])
        # pod 8 (20 000 groups: every oracle Check scans them all): its row is the groups' members; the oracle confirms the row and a sample outside it
        row8 = ids_of(bms[8])
        assert row8 == set(gu_s.tolist()) and len(row8) > 15000
        probe = np.unique(np.concatenate([np.fromiter(row8, dtype=np.uint32), rng.integers(0, nu, size=3000).astype(np.uint32)]))
        p, err = o.check_bulk_ids_mt(8, "pod", "view", np.full(probe.size, 8, dtype=np.uint32), "user", "", probe)
        assert not err.any() and set(probe[p == PERM_HAS].tolist()) == row8
        bms, _, _ = e.lookup_subjects_ids_batch("pod", "view", "group", "member", rids[8:])
        assert ids_of(bms[0]) == set(range(ngroup))


def test_string_form(aclgpu):
    with aclgpu.Engine(SCHEMA_WILD, device=0) as e:
        e.touch(*WILD_RELS)
        e.touch(("doc", "ns/with-slash", "viewer", "user", "name/with|odd=chars", ""))
        assert e.lookup_subjects("doc", "ns/with-slash", "view", "user") == ({"name/with|odd=chars"}, False, set())
        bm, cnt, wild, ex = e.lookup_subjects_bitmap("doc", "d2", "view", "user")
        assert set(e.bitmap_names("user", bm)) == {"u1", "u3"} and cnt == 2 and not wild and ex is None
        assert e.lookup_subjects("doc", "never-written", "view", "user") == (set(), False, set())
        with pytest.raises(aclgpu.AclError) as x:
            e.lookup_subjects("doc", "d1", "no_such_permission", "user")
        assert x.value.code == aclgpu.ERR_FAILED_PRECONDITION
        with pytest.raises(aclgpu.AclError) as x:
            e.lookup_subjects("no_such_type", "d1", "view", "user")
        assert x.value.code == aclgpu.ERR_FAILED_PRECONDITION
        for bad in ("bad id", "*", ""):
            with pytest.raises(aclgpu.AclError) as x:
                e.lookup_subjects("doc", bad, "view", "user")
            assert x.value.code == aclgpu.ERR_INVALID_ARGUMENT
        with pytest.raises(aclgpu.AclError) as x:
            e.lookup_subjects_ids_batch("doc", "view", "user", "", [e.object_count("doc") + 5])
        assert x.value.code == aclgpu.ERR_INVALID_ARGUMENT

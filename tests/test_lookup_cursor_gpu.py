"""Paged lookups on the GPU (acl_lookup_cursor_*, kernels.hip k_rows_page_plan / k_rows_page).  The yardstick is never the new code: the rows are those of
the existing batch calls on the same snapshot, the id sets those of both oracles (oracle.orc, oracle.pyoracle), and for a row with sorted id list S every
request must return exactly ids == [x for x in S if x > after][:limit] and more == (len([x for x in S if x > after]) > limit)."""
import numpy as np
import pytest

from oracle import orc
from oracle.pyoracle import HAS, PyOracle

pytestmark = pytest.mark.gpu

PERM_HAS = 2
LAUNCHES_PER_CALL = 2  # documented (include/aclgpu.h acl_lookup_cursor_stats): a plan launch and the page launch, whatever m is


@pytest.fixture(scope="module")
def aclgpu(aclgpu_lib):
    import aclgpu as m
    return m


def ids_of(row):
    return np.flatnonzero(np.unpackbits(np.ascontiguousarray(row, dtype=np.uint32).view(np.uint8), bitorder="little")).astype(np.int64)


def want_page(S, after, limit):
    rest = [x for x in S if after is None or x > after]
    return rest[:limit], len(rest) > limit


def check_requests(cur, reqs, rows):
    """one pages call for all of reqs [(row, after, limit)]; every answer against the id lists rows[row]"""
    got = cur.pages(reqs)
    assert len(got) == len(reqs)
    for (row, after, limit), (ids, more) in zip(reqs, got):
        w_ids, w_more = want_page(rows[row], after, limit)
        assert ids.tolist() == w_ids and more == w_more, (row, after, limit, ids.tolist()[:8], w_ids[:8], more, w_more)


def chain(cur, row, limit):
    """every page of a row, the next `after` the last id returned"""
    out, after = [], None
    for _ in range(1 << 20):
        ids, more = cur.page(row, after, limit)
        out += ids.tolist()
        if not more:
            return out
        assert ids.size == limit
        after = int(ids[-1])
    raise AssertionError("the pages never end")


def hand_graph():
    """C4's schema: three users, groups nested three deep (and one group#member subject), two namespaces, six pods (tests/test_lookup_multi_gpu.py hand_graph)"""
    rels = [("group", "g1", "member", "user", "ann", ""), ("group", "g2", "member", "group", "g1", "member"), ("group", "g3", "member", "group", "g2", "member"),
            ("group", "g3", "member", "user", "bob", ""), ("group", "side", "member", "user", "cy", ""),
            ("namespace", "n1", "viewer", "group", "g3", "member"), ("namespace", "n1", "creator", "user", "cy", ""), ("namespace", "n2", "viewer", "user", "ann", ""),
            ("namespace", "n2", "creator", "user", "bob", "")]
    for p in range(6):
        rels.append(("pod", f"p{p}", "namespace", "namespace", "n1" if p < 4 else "n2", ""))
    rels += [("pod", "p0", "viewer", "user", "ann", ""), ("pod", "p4", "viewer", "group", "g2", "member"), ("pod", "p5", "viewer", "group", "side", "member"),
             ("pod", "p1", "creator", "user", "bob", ""), ("pod", "p5", "creator", "user", "ann", ""), ("pod", "p2", "viewer", "user", "cy", "")]
    return rels


def oracles(schema, rels):
    co, po = orc.Oracle(schema), PyOracle(schema)
    co.write([(orc.OP_TOUCH, r) for r in rels])
    for r in rels:
        po.touch(*r)
    return co, po


def subject_names(e, st):
    return [n for n in (e.object_name(st, i) for i in range(e.object_count(st))) if n and n != "*"]


def test_hand_graph_both_directions(aclgpu):
    from aclgpu import workloads
    schema, rels = workloads.SCHEMA_C4, hand_graph()
    co, po = oracles(schema, rels)
    with aclgpu.Engine(schema) as e:
        e.write([(aclgpu.OP_TOUCH, r) for r in rels])
        subjects = [("user", "", ["ann", "bob", "cy", "nobody"]), ("group", "member", ["g1", "g2", "side"])]
        # LookupResources rows
        for stype, srel, names in subjects:
            sids = [e.intern(stype, n) for n in names]
            for rt, pm in (("pod", "view"), ("namespace", "view"), ("group", "member")):
                bms, counts = e.lookup_ids_batch(rt, pm, stype, srel, sids)
                with e.lookup_cursor(rt, pm, stype, srel, sids) as cur:
                    rev, ccounts, flags = cur.info()
                    assert rev == e.revision and ccounts.tolist() == counts.tolist() and not flags.any()
                    rows = [ids_of(b).tolist() for b in bms]
                    for i, n in enumerate(names):
                        S = rows[i]
                        want = co.lookup(rt, pm, stype, n, srel)
                        assert want == po.lookup_resources(rt, pm, stype, n, srel)
                        for limit in sorted({1, 2, max(len(S), 1), len(S) + 1}):
                            got = chain(cur, i, limit)
                            assert got == S and {e.object_name(rt, x) for x in got} == want, (rt, pm, stype, n, limit)
                            check_requests(cur, [(i, a, limit) for a in [None] + S + [x - 1 for x in S if x] + [10 ** 6]], rows)
                        ids, nm, more = cur.page_names(i, None, len(S) + 1)
                        assert ids.tolist() == S and nm == [e.object_name(rt, x) for x in S] and set(nm) == want and not more
                        if len(S) > 1:
                            ids, nm, more = cur.page_names(i, S[0], 1)
                            assert ids.tolist() == S[1:2] and nm == [e.object_name(rt, S[1])] and more == (len(S) > 2)
        # the launches of a pages call do not depend on its size
        ann = e.intern("user", "ann")
        with e.lookup_cursor("pod", "view", "user", "", [ann, ann]) as cur:
            for reqs in ([(0, None, 3)], [(k % 2, None, 1 + k) for k in range(7)], [(1, 2, 2)] * 40):
                before = e.stats()["page_launches"]
                cur.pages(reqs)
                assert e.stats()["page_launches"] - before == LAUNCHES_PER_CALL
            before = e.stats()["page_launches"]
            assert cur.pages([]) == [] and e.stats()["page_launches"] == before  # (m == 0: nothing runs)
        # LookupSubjects rows
        pods = [f"p{p}" for p in range(6)] + ["nsx"]
        rids = [e.intern("pod", p) for p in pods]
        for stype, srel in (("user", ""), ("group", "member")):
            names = subject_names(e, stype)
            bms, counts, bflags = e.lookup_subjects_ids_batch("pod", "view", stype, srel, rids)
            with e.subjects_cursor("pod", "view", stype, srel, rids) as cur:
                _rev, ccounts, flags = cur.info()
                assert ccounts.tolist() == counts.tolist() and flags.tolist() == bflags.tolist() and cur.row_type == stype
                rows = [ids_of(b).tolist() for b in bms]
                for i, p in enumerate(pods):
                    S = rows[i]
                    want = {s for s in names if co.check("pod", p, "view", stype, s, srel) == (PERM_HAS, 0)}
                    assert want == {s for s in names if po.check("pod", p, "view", stype, s, srel) == HAS}
                    for limit in sorted({1, 2, max(len(S), 1), len(S) + 1}):
                        got = chain(cur, i, limit)
                        assert got == S and {e.object_name(stype, x) for x in got} == want, (p, stype, limit)
                    ids, nm, _more = cur.page_names(i, None, len(S) + 1)
                    assert ids.tolist() == S and set(nm) == want
            assert sum(len(r) for r in rows) > 0


SCHEMA_EDGES = """
definition user {}
definition doc { relation viewer: user
 permission view = viewer }
definition note { relation viewer: user
 permission view = viewer }
definition solo { relation viewer: user
 permission view = viewer }
"""
# per user: the docs held.  31..33: a word edge; 8 191 / 8 192: a step edge (256 words); 131 071..131 073: a tile edge (kDiffTileWords x 32); a sparse row whose
# pages jump from tile to tile; a row with two whole empty tiles between its two ids (the type has 400 001 ids: four tiles)
EDGE_SETS = [[0], [31, 32, 33], [8191, 8192], [131071, 131072, 131073], [5, 131080, 300000], [7, 400000], [0, 31, 32, 8191, 8192, 131071, 131072, 262143, 262144, 400000]]
N_NOTES = 9000


@pytest.fixture(scope="module")
def edge_engine(aclgpu):
    with aclgpu.Engine(SCHEMA_EDGES) as e:
        for u, S in enumerate(EDGE_SETS):
            e.add_edges("doc", "viewer", "user", "", np.array(S, dtype=np.uint32), np.full(len(S), u, dtype=np.uint32))
        e.add_edges("note", "viewer", "user", "", np.arange(N_NOTES, dtype=np.uint32), np.zeros(N_NOTES, dtype=np.uint32))
        e.add_edges("solo", "viewer", "user", "", np.array([0, 0], dtype=np.uint32), np.array([1, len(EDGE_SETS)], dtype=np.uint32))  # (the last user exists and holds no doc)
        yield e


def test_row_shape_edges(aclgpu, edge_engine):
    e = edge_engine
    users = list(range(len(EDGE_SETS))) + [len(EDGE_SETS)]  # (the last one holds nothing)
    rows = EDGE_SETS + [[]]
    nobj = e.object_count("doc")
    assert nobj == 400001
    bms, counts = e.lookup_ids_batch("doc", "view", "user", "", users)
    assert [ids_of(b).tolist() for b in bms] == rows  # (the truth is the id list itself, and the batch call agrees)
    with e.lookup_cursor("doc", "view", "user", "", users) as cur:
        assert cur.info()[1].tolist() == counts.tolist() == [len(S) for S in rows]
        edges = sorted({x for S in EDGE_SETS for x in S})
        afters = {None, 0, 1, 100000, 200000, 262143, 262144, 399999, 400000, 400001, nobj + 31, nobj + 5000, 1 << 20, 0xFFFFFFFE}
        for x in edges:
            afters |= {max(x - 1, 0), x, x + 1}
        afters = sorted(afters, key=lambda a: -1 if a is None else a)
        for i, S in enumerate(rows):
            for limit in sorted({1, 2, 3, len(S) + 1}):
                check_requests(cur, [(i, a, limit) for a in afters], rows)
            assert chain(cur, i, 1) == S and chain(cur, i, 4) == S
    # a dense row: one user holds every note
    dense = [list(range(N_NOTES))]
    with e.lookup_cursor("note", "view", "user", "", [0]) as cur:
        assert cur.info()[1].tolist() == [N_NOTES]
        afters = [None, 0, 30, 31, 32, 63, 4095, 4096, 8190, 8191, 8192, 8997, 8998, 8999, 9000, 20000]
        for limit in (1, 64, 4096, 9000):
            check_requests(cur, [(0, a, limit) for a in afters], dense)
        assert chain(cur, 0, 4096) == dense[0] and chain(cur, 0, 8999) == dense[0]
    # a type with a single object
    with e.lookup_cursor("solo", "view", "user", "", [1, 0]) as cur:
        assert cur.info()[1].tolist() == [1, 0]
        check_requests(cur, [(r, a, limit) for r in (0, 1) for a in (None, 0, 1, 31, 32, 127, 128, 5000) for limit in (1, 5)], [[0], []])


def test_many_requests_in_one_call(aclgpu, edge_engine):
    """300 requests over 7 rows, rows repeated and shuffled, mixed limits: every answer at its prefix-of-limits offset, the words behind n_out[q] untouched"""
    e = edge_engine
    rng = np.random.default_rng(20261020)
    users = list(range(7))
    rows = EDGE_SETS[:7]
    with e.lookup_cursor("doc", "view", "user", "", users) as cur:
        m = 300
        reqs = np.zeros((m, 4), dtype=np.uint32)
        reqs[:, 0] = rng.integers(0, 7, size=m)
        pool = np.array(sorted({x + d for S in rows for x in S for d in (-1, 0, 1) if x + d >= 0} | {aclgpu.PAGE_FROM_START, 50000, 390000, 500000}), dtype=np.uint32)
        reqs[:, 1] = rng.choice(pool, size=m)
        reqs[::3, 1] = aclgpu.PAGE_FROM_START
        reqs[:, 2] = rng.choice([1, 2, 3, 5, 11, 64, 700], size=m)
        off = np.concatenate(([0], np.cumsum(reqs[:, 2], dtype=np.int64)))
        SENT = 0xDEADBEEF
        ids = np.full(int(off[-1]) + 8, SENT, dtype=np.uint32)
        n, more = np.full(m, SENT, dtype=np.uint32), np.full(m, 0xEE, dtype=np.uint8)
        before = e.stats()["page_launches"]
        e._check(e._L.acl_lookup_cursor_pages(e._h, cur._c, reqs.ctypes.data, m, ids.ctypes.data, int(off[-1]), n.ctypes.data, more.ctypes.data, None))
        assert e.stats()["page_launches"] - before == LAUNCHES_PER_CALL
        assert (ids[int(off[-1]):] == SENT).all()
        for q in range(m):
            row, after, limit = int(reqs[q, 0]), int(reqs[q, 1]), int(reqs[q, 2])
            w_ids, w_more = want_page(rows[row], None if after == aclgpu.PAGE_FROM_START else after, limit)
            assert int(n[q]) == len(w_ids) and int(more[q]) == int(w_more), (q, row, after, limit)
            assert ids[off[q]:off[q] + len(w_ids)].tolist() == w_ids, (q, row, after, limit)
            assert (ids[off[q] + len(w_ids):off[q + 1]] == SENT).all(), (q, row, after, limit)
        assert sum(int(x) for x in n) > 100 and int(more.sum()) > 10
        # an ids_cap one short, and a row beyond the cursor's: refused, nothing written
        ids[:] = SENT
        assert e._L.acl_lookup_cursor_pages(e._h, cur._c, reqs.ctypes.data, m, ids.ctypes.data, int(off[-1]) - 1, n.ctypes.data, more.ctypes.data, None) == aclgpu.ERR_INVALID_ARGUMENT
        reqs[150, 0] = 7
        assert e._L.acl_lookup_cursor_pages(e._h, cur._c, reqs.ctypes.data, m, ids.ctypes.data, int(off[-1]), n.ctypes.data, more.ctypes.data, None) == aclgpu.ERR_INVALID_ARGUMENT
        assert b"row 7" in e._L.acl_last_error() and (ids == SENT).all()


def all_pages(cur, n_rows, limit=3):
    return [chain(cur, i, limit) for i in range(n_rows)]


def test_the_cursor_is_pinned(aclgpu):
    from aclgpu import workloads
    schema, rels = workloads.SCHEMA_C4, hand_graph()
    co, po = oracles(schema, rels)
    with aclgpu.Engine(schema) as e:
        e.write([(aclgpu.OP_TOUCH, r) for r in rels])
        names = ["ann", "bob", "cy"]
        sids = [e.intern("user", n) for n in names]
        cur = e.lookup_cursor("pod", "view", "user", "", sids)
        scur = e.subjects_cursor("pod", "view", "user", "", [e.intern("pod", "p2"), e.intern("pod", "p5")])
        rev0, counts0, _ = cur.info()
        pages0, spages0, sinfo0 = all_pages(cur, 3), all_pages(scur, 2), scur.info()
        assert [{e.object_name("pod", x) for x in p} for p in pages0] == [co.lookup("pod", "view", "user", n) for n in names]
        nobj0 = e.object_count("pod")
        # a grant of a new resource, the delete of a granted one, and the type widened by more than 32 ids (one of the new ids granted, too)
        ups = [(aclgpu.OP_TOUCH, ("pod", "p9", "viewer", "user", "cy", "")), (aclgpu.OP_DELETE, ("pod", "p2", "viewer", "user", "cy", "")),
               (aclgpu.OP_DELETE, ("group", "side", "member", "user", "cy", ""))]
        e.write(ups)
        for i in range(40):
            e.intern("pod", f"wide{i}")
        late = [(aclgpu.OP_TOUCH, ("pod", "wide39", "creator", "user", "cy", "")), (aclgpu.OP_TOUCH, ("pod", "wide39", "viewer", "user", "bob", ""))]
        e.write(late)
        assert e.object_count("pod") >= nobj0 + 41 and e.revision > rev0
        co.write([(orc.OP_TOUCH if op == aclgpu.OP_TOUCH else orc.OP_DELETE, r) for op, r in ups + late])
        for op, r in ups + late:
            po.touch(*r) if op == aclgpu.OP_TOUCH else po.delete(*r)
        e.lookup_ids_batch("pod", "view", "user", "", sids)  # (the snapshot moves on under the cursors)
        rev1, counts1, _ = cur.info()
        assert rev1 == rev0 and counts1.tolist() == counts0.tolist() and all_pages(cur, 3) == pages0
        assert all_pages(scur, 2) == spages0 and [x.tolist() if hasattr(x, "tolist") else x for x in scur.info()] == [x.tolist() if hasattr(x, "tolist") else x for x in sinfo0]
        # a fresh cursor: the new answer, equal to the batch call and both oracles
        with e.lookup_cursor("pod", "view", "user", "", sids) as fresh:
            assert fresh.info()[0] == e.revision > rev0
            now = all_pages(fresh, 3)
            assert now != pages0
            bms, _ = e.lookup_ids_batch("pod", "view", "user", "", sids)
            for i, n in enumerate(names):
                want = co.lookup("pod", "view", "user", n)
                assert want == po.lookup_resources("pod", "view", "user", n)
                assert now[i] == ids_of(bms[i]).tolist() and {e.object_name("pod", x) for x in now[i]} == want
            assert "wide39" in {e.object_name("pod", x) for x in now[2]} and "p9" in {e.object_name("pod", x) for x in now[2]}
        with e.subjects_cursor("pod", "view", "user", "", [e.intern("pod", "p2"), e.intern("pod", "p5")]) as fresh:
            now = all_pages(fresh, 2)
            assert now != spages0
            for i, p in enumerate(("p2", "p5")):
                want = {s for s in subject_names(e, "user") if co.check("pod", p, "view", "user", s) == (PERM_HAS, 0)}
                assert want == {s for s in subject_names(e, "user") if po.check("pod", p, "view", "user", s) == HAS}
                assert {e.object_name("user", x) for x in now[i]} == want
        cur.close()
        scur.close()


SCHEMA_LIVE = """
definition user {}
definition doc {
  relation viewer: user with expiration
  permission view = viewer
}
"""


def test_an_expiry_does_not_move_an_open_cursor(aclgpu):
    with aclgpu.Engine(SCHEMA_LIVE) as e:
        e.set_now(10)
        e.write([(aclgpu.OP_TOUCH, ("doc", f"d{i}", "viewer", "user", "u", ""), 100 if i % 2 else 0) for i in range(6)])
        u = e.intern("user", "u")
        with e.lookup_cursor("doc", "view", "user", "", [u]) as cur:
            before = chain(cur, 0, 2)
            assert len(before) == 6
            e.set_now(200)
            assert e.lookup("doc", "view", "user", "u") == {"d0", "d2", "d4"}
            assert chain(cur, 0, 2) == before and cur.info()[1].tolist() == [6]
            with e.lookup_cursor("doc", "view", "user", "", [u]) as fresh:
                assert {e.object_name("doc", x) for x in chain(fresh, 0, 2)} == {"d0", "d2", "d4"}


def test_a_recycled_id_expires_the_names_not_the_ids(aclgpu, monkeypatch):
    """ACL_ID_QUARANTINE_MS=0 (the test knob of tests/test_write_path_gpu.py): a pod that loses its only relationship hands its id to the next new pod.  The
    cursor's ids stay what they were; names are refused from then on, because the id no longer carries the name it had at the cursor's revision."""
    from tests import kat_runner
    b = kat_runner.load_bootstrap()
    monkeypatch.setenv("ACL_ID_QUARANTINE_MS", "0")
    with aclgpu.Engine(b["schema"], "\n".join(b["relationships"])) as e:
        e.write([(aclgpu.OP_TOUCH, ("pod", f"ns/p{i}", "creator", "user", "paul", "")) for i in range(5)])
        paul = e.intern("user", "paul")
        with e.lookup_cursor("pod", "view", "user", "", [paul]) as cur:
            ids, names, more = cur.page_names(0, None, 10)
            assert sorted(names) == [f"ns/p{i}" for i in range(5)] and not more and names == [e.object_name("pod", int(x)) for x in ids]
            old = e.find("pod", "ns/p3")
            assert e.delete_by_filter(rtype="pod", rid="ns/p3") == 1
            e.write([(aclgpu.OP_TOUCH, ("pod", "ns/brand-new", "creator", "user", "chani", ""))])
            assert e.find("pod", "ns/brand-new") == old and e.stats()["ids_recycled"] == 1
            with pytest.raises(aclgpu.AclError) as ei:
                cur.page_names(0, None, 10)
            assert ei.value.code == aclgpu.ERR_FAILED_PRECONDITION and "reopen" in ei.value.message
            again, more = cur.page(0, None, 10)
            assert again.tolist() == ids.tolist() and not more and cur.info()[1].tolist() == [5]
        with e.lookup_cursor("pod", "view", "user", "", [paul]) as fresh:  # reopened: names again
            assert sorted(fresh.page_names(0, None, 10)[1]) == [f"ns/p{i}" for i in (0, 1, 2, 4)]


SCHEMA_NONMONO = """
definition user {}
definition group { relation member: user | group#member }
definition doc {
  relation viewer: user | user:* | group#member
  relation banned: user
  permission view = viewer - banned
}
"""


def test_exclusion_and_wildcard(aclgpu):
    rels = [("group", "g", "member", "user", "u1", ""), ("group", "g", "member", "user", "u2", ""), ("doc", "team", "viewer", "group", "g", "member"),
            ("doc", "team", "banned", "user", "u2", ""), ("doc", "open", "viewer", "user", "*", ""), ("doc", "open", "viewer", "user", "u3", ""),
            ("doc", "open", "banned", "user", "u1", ""), ("doc", "open", "banned", "user", "u3", ""), ("doc", "mine", "viewer", "user", "u4", ""),
            ("doc", "open", "viewer", "user", "u5", "")]
    rels += [("doc", f"d{i}", "viewer", "user", "u1", "") for i in range(40)] + [("doc", f"d{i}", "banned", "user", "u1", "") for i in range(0, 40, 3)]
    co, po = oracles(SCHEMA_NONMONO, rels)
    relaxed = PyOracle(SCHEMA_NONMONO)  # LookupSubjects' reach: the positive relaxation on the relationships minus the `user:*` ones (tests/test_lookup_subjects_gpu.py)
    for r in rels:
        if r[4] != "*":
            relaxed.touch(*r)
    relaxed.relaxed = True
    with aclgpu.Engine(SCHEMA_NONMONO) as e:
        e.write([(aclgpu.OP_TOUCH, r) for r in rels])
        users = ["u1", "u2", "u3", "u4", "u5", "stranger"]
        sids = [e.intern("user", n) for n in users]
        bms, counts = e.lookup_ids_batch("doc", "view", "user", "", sids)
        with e.lookup_cursor("doc", "view", "user", "", sids) as cur:
            assert cur.info()[1].tolist() == counts.tolist()
            for i, n in enumerate(users):
                want = co.lookup("doc", "view", "user", n)
                assert want == po.lookup_resources("doc", "view", "user", n)
                for limit in (1, 7, 64):
                    got = chain(cur, i, limit)
                    assert got == ids_of(bms[i]).tolist() and {e.object_name("doc", x) for x in got} == want, (n, limit)
        docs = ["team", "open", "mine", "d0", "d1"]
        rids = [e.intern("doc", d) for d in docs]
        bms, counts, bflags = e.lookup_subjects_ids_batch("doc", "view", "user", "", rids)
        with e.subjects_cursor("doc", "view", "user", "", rids) as cur:
            _rev, ccounts, flags = cur.info()
            assert ccounts.tolist() == counts.tolist() and flags.tolist() == bflags.tolist() == [0, 1, 0, 0, 0]  # ACL_SUBJECTS_WILDCARD on `open`
            for i, d in enumerate(docs):
                want = {s for s in users if relaxed.check("doc", d, "view", "user", s) == HAS and po.check("doc", d, "view", "user", s) == HAS}
                assert want == {s for s in users if relaxed.check("doc", d, "view", "user", s) == HAS and co.check("doc", d, "view", "user", s) == (PERM_HAS, 0)}
                for limit in (1, 2, 9):
                    got = chain(cur, i, limit)
                    assert got == ids_of(bms[i]).tolist() and {e.object_name("user", x) for x in got} == want, (d, limit)
            assert {e.object_name("user", x) for x in chain(cur, 1, 4)} == {"u5"}  # (named on `open` and not banned; the wildcard itself is the flag, not a bit)


DEPTH_SCHEMA = """
definition user {}
definition group { relation member: user | group#member }
definition doc {
  relation viewer: user | group#member
  relation owner: user
  relation banned: user | group#member
  permission view = viewer + owner
  permission seen = view - banned
}
"""


@pytest.mark.parametrize("lenient", [False, True])
def test_depth_limit_open_answers_as_the_batch_call(aclgpu, lenient):
    """the 55-group chain of tests/test_lookup_multi_gpu.py test_depth_limit_each_target_keeps_its_own_rule, plus one doc that `deep` views directly and whose ban
    hangs on the top of the chain: `seen` confirms its candidates by a forward Check, and that doc's runs into the depth limit under `banned`.  The open fails or
    succeeds exactly as the batch call, and on success the pages are its row"""
    rels = [("group", "g1", "member", "user", "deep", "")] + [("group", f"g{i + 1}", "member", "group", f"g{i}", "member") for i in range(1, 55)]
    rels += [("doc", f"d{k}", "viewer", "group", f"g{k}", "member") for k in range(40, 56)] + [("doc", "direct", "viewer", "user", "deep", ""), ("doc", "own", "owner", "user", "deep", "")]
    rels += [("doc", "bad", "viewer", "user", "deep", ""), ("doc", "bad", "banned", "group", "g55", "member")]
    outcomes = {}
    with aclgpu.Engine(DEPTH_SCHEMA, lenient_lookup=lenient) as e:
        e.write([(aclgpu.OP_TOUCH, r) for r in rels])
        deep = e.intern("user", "deep")
        d55, bad = e.intern("doc", "d55"), e.intern("doc", "bad")
        calls = [("res", t, (lambda t=t: e.lookup_ids_batch(t[0], t[1], "user", "", [deep])[0]), (lambda t=t: e.lookup_cursor(t[0], t[1], "user", "", [deep])))
                 for t in (("doc", "view"), ("doc", "viewer"), ("group", "member"), ("doc", "seen"))]
        calls += [("subj", t + (r,), (lambda t=t, r=r: e.lookup_subjects_ids_batch(t[0], t[1], "user", "", [r])[0]), (lambda t=t, r=r: e.subjects_cursor(t[0], t[1], "user", "", [r])))
                  for t in (("doc", "view"), ("doc", "seen")) for r in (d55, bad)]
        for kind, t, batch, open_ in calls:
            try:
                row = ids_of(batch()[0]).tolist()
            except aclgpu.AclError as x:
                with pytest.raises(aclgpu.AclError) as ei:
                    open_()
                assert ei.value.code == x.code == aclgpu.ERR_DEPTH, (kind, t)
                outcomes[(kind, t)] = "DEPTH"
                continue
            with open_() as cur:
                assert chain(cur, 0, 4) == row and cur.info()[1].tolist() == [len(row)], (kind, t)
            outcomes[(kind, t)] = len(row)
    print("depth outcomes", lenient, outcomes)
    assert outcomes[("res", ("doc", "view"))] == 12 and outcomes[("res", ("doc", "viewer"))] == 12 and outcomes[("res", ("group", "member"))] == 50
    # (lookups.go:75-83: a candidate's Check error fails the stream; ACL_FLAG_LENIENT_LOOKUP leaves the candidate out)
    assert outcomes[("res", ("doc", "seen"))] == (10 if lenient else "DEPTH")
    assert outcomes[("subj", ("doc", "seen", bad))] == (0 if lenient else "DEPTH") and outcomes[("subj", ("doc", "view", bad))] == 1


def test_two_replicas_rows_live_on_one_of_them(aclgpu):
    """an engine with two logical replicas on one GPU: every cursor's rows live on one replica's device and its pages run there, whichever replica answered last"""
    from aclgpu import workloads
    schema, rels = workloads.SCHEMA_C4, hand_graph()
    co, _po = oracles(schema, rels)
    with aclgpu.Engine(schema, devices=[0, 0]) as e:
        e.write([(aclgpu.OP_TOUCH, r) for r in rels])
        names = ["ann", "bob", "cy"]
        sids = [e.intern("user", n) for n in names]
        curs = [e.lookup_cursor("pod", "view", "user", "", sids) for _ in range(3)] + [e.subjects_cursor("pod", "view", "user", "", [e.intern("pod", "p5")])]
        for _ in range(3):  # (lookups in between land on both replicas)
            e.lookup_ids_batch("pod", "view", "user", "", sids)
            for cur in curs[:3]:
                for i, n in enumerate(names):
                    assert {e.object_name("pod", x) for x in chain(cur, i, 2)} == co.lookup("pod", "view", "user", n)
            assert {e.object_name("user", x) for x in chain(curs[3], 0, 1)} == {s for s in names if co.check("pod", "p5", "view", "user", s) == (PERM_HAS, 0)}
        for cur in curs:
            cur.close()


def code_of(aclgpu, call):
    with pytest.raises(aclgpu.AclError) as ei:
        call()
    return ei.value.code


def test_lifetime(aclgpu, aclgpu_lib):
    from aclgpu import workloads
    L = aclgpu_lib
    schema, rels = workloads.SCHEMA_C4, hand_graph()
    with aclgpu.Engine(schema) as e:
        e.write([(aclgpu.OP_TOUCH, r) for r in rels])
        ann = e.intern("user", "ann")
        # n == 0: a valid cursor without rows
        with e.lookup_cursor("pod", "view", "user", "", []) as empty:
            assert empty.info()[1].size == 0 and empty.pages([]) == []
            assert code_of(aclgpu, lambda: empty.page(0, None, 1)) == aclgpu.ERR_INVALID_ARGUMENT
        # double close
        cur = e.lookup_cursor("pod", "view", "user", "", [ann])
        handle = cur._c
        assert cur.page(0, None, 2)[0].size == 2
        cur.close()
        assert L.acl_lookup_cursor_close(e._h, handle) == aclgpu.ERR_INVALID_ARGUMENT and b"not an open cursor" in L.acl_last_error()
        ids, n, more = np.zeros(4, dtype=np.uint32), np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint8)
        rq = np.array([[0, aclgpu.PAGE_FROM_START, 4, 0]], dtype=np.uint32)
        assert L.acl_lookup_cursor_pages(e._h, handle, rq.ctypes.data, 1, ids.ctypes.data, 4, n.ctypes.data, more.ctypes.data, None) == aclgpu.ERR_INVALID_ARGUMENT
        # a cursor of ANOTHER engine is not one of this engine's
        with aclgpu.Engine(schema) as other:
            other.write([(aclgpu.OP_TOUCH, r) for r in rels])
            oc = other.lookup_cursor("pod", "view", "user", "", [other.intern("user", "ann")])
            assert L.acl_lookup_cursor_close(e._h, oc._c) == aclgpu.ERR_INVALID_ARGUMENT
            assert oc.page(0, None, 9)[0].size == 6
            oc.close()
        # a sharded engine refuses the open
        e._check(L.acl_shard_configure(e._h, 0, 2))
        assert code_of(aclgpu, lambda: e.lookup_cursor("pod", "view", "user", "", [ann])) == aclgpu.ERR_FAILED_PRECONDITION
        assert code_of(aclgpu, lambda: e.subjects_cursor("pod", "view", "user", "", [0])) == aclgpu.ERR_FAILED_PRECONDITION
        e._check(L.acl_shard_configure(e._h, 0, 1))
        # a schema reload expires an open cursor: every call but close
        cur = e.lookup_cursor("pod", "view", "user", "", [ann])
        assert cur.page(0, None, 9)[0].size == 6
        e.load_bootstrap(schema)
        for call in (cur.info, lambda: cur.page(0, None, 9), lambda: cur.page_names(0, None, 9), lambda: cur.pages([])):
            assert code_of(aclgpu, call) == aclgpu.ERR_FAILED_PRECONDITION
        cur.close()
    # closing the engine with cursors open (a resource cursor, a subject cursor, an empty one)
    e = aclgpu.Engine(schema)
    e.write([(aclgpu.OP_TOUCH, r) for r in rels])
    curs = [e.lookup_cursor("pod", "view", "user", "", [e.intern("user", "ann")]), e.subjects_cursor("pod", "view", "user", "", [e.intern("pod", "p0")]),
            e.lookup_cursor("pod", "view", "user", "", [])]
    assert curs[0].page(0, None, 9)[0].size == 6 and curs[1].page(0, None, 9)[0].size > 0
    e.close()
    for c in curs:
        c.close()  # (the handle went with the engine: nothing to do, nothing touched)
    with aclgpu.Engine(schema) as e2:  # the device is as usable as before
        e2.write([(aclgpu.OP_TOUCH, r) for r in rels])
        with e2.lookup_cursor("pod", "view", "user", "", [e2.intern("user", "cy")]) as cur:
            assert {e2.object_name("pod", int(x)) for x in cur.page(0, None, 9)[0]} == oracles(schema, rels)[0].lookup("pod", "view", "user", "cy") == {"p0", "p1", "p2", "p3", "p5"}

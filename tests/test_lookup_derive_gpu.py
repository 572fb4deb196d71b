"""Derived lookup cursors on the GPU (acl_lookup_cursor_open_mixed / _derive / _count, kernels.hip k_rows_derive).  The yardstick is never the new code: the
source rows are those of lookup_ids_batch / lookup_subjects_ids_batch on the same snapshot, combined with numpy; the id sets are those of both oracles
(oracle.orc, oracle.pyoracle), combined with Python set operations; and every page of a derived row obeys want_page's rule of tests/test_lookup_cursor_gpu.py:
ids == [x for x in S if x > after][:limit], more == (len([x for x in S if x > after]) > limit)."""
import numpy as np
import pytest

from oracle import orc
from oracle.pyoracle import HAS
from tests.test_lookup_cursor_gpu import EDGE_SETS, SCHEMA_NONMONO, chain, check_requests, hand_graph, ids_of, oracles, subject_names

pytestmark = pytest.mark.gpu

PERM_HAS = 2
LAUNCHES_PER_DERIVE = 2  # documented (include/aclgpu.h acl_lookup_derive_stats): the combine launch and the scan, whatever the sizes are
TILE_IDS = 4096 * 32     # kDiffTileWords words of 32 ids
BUDGET = 1 << 30         # the rows of all open cursors of an engine, at most (include/aclgpu.h "paged lookups")


@pytest.fixture(scope="module")
def aclgpu(aclgpu_lib):
    import aclgpu as m
    return m


def code_of(aclgpu, call):
    with pytest.raises(aclgpu.AclError) as ei:
        call()
    return ei.value.code


def row_bytes_of(nobj):
    """bytes of one row kept on the device: whole 16-byte pieces, at least one"""
    return max(4, ((nobj + 31) // 32 + 3) // 4 * 4) * 4


def bits_of(row, nobj):
    """a batch call's row as a boolean vector over the type's ids"""
    return np.unpackbits(np.ascontiguousarray(row, dtype=np.uint32).view(np.uint8), bitorder="little")[:nobj].astype(bool)


def combine(rows, any_, all_, none, nobj):
    """the yardstick: A & B & ~C over boolean vectors, with numpy"""
    r = np.zeros(nobj, dtype=bool) if any_ else np.ones(nobj, dtype=bool)
    for k in any_:
        r |= rows[k]
    for k in all_:
        r &= rows[k]
    for k in none:
        r &= ~rows[k]
    return r


def whole_rows(cur, counts):
    """every row of a cursor in ONE pages call (limit = the row's count + 1) -> [ids]; more must be False everywhere"""
    got = cur.pages([(i, None, int(c) + 1) for i, c in enumerate(counts)])
    assert not any(more for _ids, more in got)
    return [ids for ids, _more in got]


def check_derived(e, cur, want, counts=None):
    """a derived cursor against the boolean vectors `want`: info's counts, count_rows' counts if given, and every id of every row"""
    _rev, ccounts, flags = cur.info()
    assert ccounts.tolist() == [int(w.sum()) for w in want] and not flags.any()
    if counts is not None:
        assert counts.tolist() == ccounts.tolist()
    for i, ids in enumerate(whole_rows(cur, ccounts)):
        assert np.array_equal(ids, np.flatnonzero(want[i])), i


PRINCIPALS = [[("user", "", "ann")], [("user", "", "bob"), ("group", "member", "g1")], [("user", "", "cy"), ("group", "member", "side"), ("group", "member", "g2")],
              [("user", "", "nobody")]]


def test_principals_on_the_hand_graph(aclgpu):
    from aclgpu import workloads
    schema, rels = workloads.SCHEMA_C4, hand_graph()
    co, po = oracles(schema, rels)
    with aclgpu.Engine(schema) as e:
        e.write([(aclgpu.OP_TOUCH, r) for r in rels])
        forms = [("user", "", "ann"), ("user", "", "bob"), ("user", "", "cy"), ("user", "", "nobody"), ("group", "member", "g1"), ("group", "member", "side"),
                 ("group", "member", "g2")]
        interleaved = [forms[k] for k in (0, 4, 1, 5, 5, 2, 6, 3, 0)]  # (runs of length one and two, a subject named twice)
        for rt, pm in (("pod", "view"), ("namespace", "view"), ("group", "member")):
            # the mixed open: every row is the per-form batch call's row
            batch = {}
            for st, srel in (("user", ""), ("group", "member")):
                names = [n for s, _r, n in forms if s == st]
                bms, counts = e.lookup_ids_batch(rt, pm, st, srel, [e.intern(st, n) for n in names])
                for n, b, c in zip(names, bms, counts):
                    batch[(st, srel, n)] = (ids_of(b).tolist(), int(c))
            for order in (forms, interleaved):
                with e.lookup_cursor_mixed(rt, pm, [(st, srel, e.intern(st, n)) for st, srel, n in order]) as cur:
                    rev, ccounts, flags = cur.info()
                    assert rev == e.revision and not flags.any() and cur.row_type == rt and ccounts.tolist() == [batch[f][1] for f in order]
                    for i, f in enumerate(order):
                        assert chain(cur, i, 3) == batch[f][0], (rt, pm, f)
            # the principals: the union of BOTH oracles' lookups, form by form
            want = []
            for p in PRINCIPALS:
                names = set()
                for st, srel, n in p:
                    one = co.lookup(rt, pm, st, n, srel)
                    assert one == po.lookup_resources(rt, pm, st, n, srel)
                    names |= one
                want.append(names)
            with e.principal_cursor(rt, pm, PRINCIPALS) as cur:
                rev, ccounts, flags = cur.info()
                assert rev == e.revision and ccounts.tolist() == [len(w) for w in want] and not flags.any() and cur.row_type == rt
                rows = []
                for p, w in enumerate(want):
                    S = sorted(e.find(rt, n) for n in w)
                    rows.append(S)
                    for limit in sorted({1, 2, max(len(S), 1), len(S) + 1}):
                        assert chain(cur, p, limit) == S, (rt, pm, p, limit)
                    ids, nm, more = cur.page_names(p, None, len(S) + 1)
                    assert ids.tolist() == S and nm == [e.object_name(rt, x) for x in S] and set(nm) == w and not more
                for p, S in enumerate(rows):
                    for limit in sorted({1, 2, max(len(S), 1), len(S) + 1}):
                        check_requests(cur, [(p, a, limit) for a in [None] + S + [x - 1 for x in S if x] + [10 ** 6]], rows)
            assert sum(len(w) for w in want) > 0 and want[3] == set()


def test_non_monotone_sources_the_union_of_answers_not_a_multi_seed_walk(aclgpu):
    """`view = viewer - banned`: u1 is banned on `team`, which u1's group may see.  The principal {u1, g#member} sees `team`, because g#member does -- the union
    of the subjects' individual answers, each confirmed by lookup_refine.  A reverse walk seeded with u1 AND g#member reaches `team` through `banned` as well as
    through `viewer` and has no one subject to confirm the candidate against: it gets this case wrong, whichever way it decides."""
    rels = [("group", "g", "member", "user", "u1", ""), ("group", "g", "member", "user", "u2", ""), ("doc", "team", "viewer", "group", "g", "member"),
            ("doc", "team", "banned", "user", "u1", ""), ("doc", "open", "viewer", "user", "*", ""), ("doc", "open", "banned", "user", "u1", ""),
            ("doc", "mine", "viewer", "user", "u1", ""), ("doc", "gone", "viewer", "user", "u1", ""), ("doc", "gone", "banned", "user", "u1", ""),
            ("doc", "other", "viewer", "user", "u2", "")]
    co, po = oracles(SCHEMA_NONMONO, rels)
    with aclgpu.Engine(SCHEMA_NONMONO) as e:
        e.write([(aclgpu.OP_TOUCH, r) for r in rels])
        principals = [[("user", "", "u1"), ("group", "member", "g")], [("user", "", "u1")], [("group", "member", "g")], [("user", "", "u2"), ("group", "member", "g")]]
        want = []
        for p in principals:
            names = set()
            for st, srel, n in p:
                one = co.lookup("doc", "view", st, n, srel)
                assert one == po.lookup_resources("doc", "view", st, n, srel)
                names |= one
            want.append(names)
        assert "team" in want[0] and "team" not in want[1] and "team" in want[2] and "open" not in want[1] and "gone" not in want[0] and "mine" in want[0]
        with e.principal_cursor("doc", "view", principals) as cur:
            assert cur.info()[1].tolist() == [len(w) for w in want]
            for p, w in enumerate(want):
                for limit in (1, 2, 64):
                    assert {e.object_name("doc", x) for x in chain(cur, p, limit)} == w, (p, limit)
        # the sources themselves are the batch call's rows, confirmed per run
        subjects = [("user", "", e.intern("user", "u1")), ("group", "member", e.intern("group", "g")), ("user", "", e.intern("user", "u2"))]
        with e.lookup_cursor_mixed("doc", "view", subjects) as cur:
            for i, (st, srel, sid) in enumerate(subjects):
                bms, counts = e.lookup_ids_batch("doc", "view", st, srel, [sid])
                assert chain(cur, i, 2) == ids_of(bms[0]).tolist() and int(cur.info()[1][i]) == int(counts[0])


SCHEMA_EDGES = """
definition user {}
definition doc { relation viewer: user
 permission view = viewer }
definition note { relation viewer: user
 permission view = viewer }
"""
N_DOCS = 400001  # four tiles
EVEN, MOD3 = len(EDGE_SETS), len(EDGE_SETS) + 1


@pytest.fixture(scope="module")
def edge_engine(aclgpu):
    """users 0..6 hold EDGE_SETS (word edges 31..33, the step edge 8191 / 8192, the tile edges 131071..131073 and 262143 / 262144, the last id 400000); two dense
    users hold every even id and every id that is 0 mod 3.  The rows are read once, by the batch call, and shared."""
    with aclgpu.Engine(SCHEMA_EDGES) as e:
        for u, S in enumerate(EDGE_SETS):
            e.add_edges("doc", "viewer", "user", "", np.array(S, dtype=np.uint32), np.full(len(S), u, dtype=np.uint32))
        even, mod3 = np.arange(0, N_DOCS, 2, dtype=np.uint32), np.arange(0, N_DOCS, 3, dtype=np.uint32)
        e.add_edges("doc", "viewer", "user", "", even, np.full(even.size, EVEN, dtype=np.uint32))
        e.add_edges("doc", "viewer", "user", "", mod3, np.full(mod3.size, MOD3, dtype=np.uint32))
        e.add_edges("note", "viewer", "user", "", np.array([0], dtype=np.uint32), np.array([0], dtype=np.uint32))
        assert e.object_count("doc") == N_DOCS
        users = list(range(len(EDGE_SETS) + 2))
        bms, _counts = e.lookup_ids_batch("doc", "view", "user", "", users)
        rows = [bits_of(b, N_DOCS) for b in bms]
        for u, S in enumerate(EDGE_SETS):
            assert np.flatnonzero(rows[u]).tolist() == S
        assert rows[EVEN].sum() == 200001 and rows[MOD3].sum() == 133334
        yield e, users, rows


def test_row_shape_edges(aclgpu, edge_engine):
    e, users, rows = edge_engine
    n = len(users)
    exprs, lists = [], []

    def add(any_, all_, none):
        lists.append((any_, all_, none))
        exprs.append(([(0, k) for k in any_], [(0, k) for k in all_], [(0, k) for k in none]))

    for i in range(n):
        for j in range(n):
            add([i, j], [], [])      # any{i, j}
            add([], [i, j], [])      # all{i, j}
            add([i], [], [j])        # i \ j (i \ i: empty)
    first_extra = len(exprs)
    for i in range(n):
        add([i], [], [])             # a single-operand copy
    add([], [EVEN, MOD3, 6], [])     # an all-only list of three
    add([], [EVEN], [MOD3, 1])       # n_any == 0 with all + none
    add([], [EVEN, MOD3], [6])
    add([0, 1, 2, 3, 4, 5, 6], [EVEN], [MOD3])
    both = len(exprs)
    add([], [EVEN, MOD3], [])        # even & mod3: every sixth id, over all four tiles
    want = [combine(rows, a, b, c, N_DOCS) for a, b, c in lists]
    assert all(not want[3 * (i * n + i) + 2].any() for i in range(n)) and want[both].sum() == 66667 and len(exprs) > first_extra
    with e.lookup_cursor("doc", "view", "user", "", users) as src:
        counts = e.count_rows([src], exprs)
        with e.derive_cursor([src], exprs) as cur:
            assert cur.row_type == "doc" and cur.info()[0] == src.info()[0]
            check_derived(e, cur, want, counts)
            # even & mod3 in pages of 4096, and from every tile edge +- 1
            S = np.flatnonzero(want[both]).tolist()
            assert chain(cur, both, 4096) == S
            table = {both: S}
            afters = [None] + [t * TILE_IDS + d for t in (1, 2, 3) for d in (-2, -1, 0, 1)] + [N_DOCS - 2, N_DOCS - 1, N_DOCS, N_DOCS + 40]
            for limit in (1, 7, 4096):
                check_requests(cur, [(both, a, limit) for a in afters], table)
            # the sparse rows at their own edges
            for k in range(len(EDGE_SETS)):
                Sk = EDGE_SETS[k]
                copy = first_extra + k
                check_requests(cur, [(copy, a, limit) for limit in (1, 3) for a in [None] + Sk + [max(x - 1, 0) for x in Sk] + [x + 1 for x in Sk]], {copy: Sk})


def test_the_derived_rows_count_towards_the_budget(aclgpu, edge_engine):
    e, users, rows = edge_engine
    row_bytes = row_bytes_of(N_DOCS)
    n_big = int(0.7 * BUDGET) // row_bytes  # two of these do not fit together
    refs = np.zeros((n_big, 2), dtype=np.uint32)
    refs[:, 1] = 5
    ex = np.zeros((n_big, 4), dtype=np.uint32)
    ex[:, 0] = np.arange(n_big)
    ex[:, 1] = 1
    with e.lookup_cursor("doc", "view", "user", "", users) as src:
        first = e.derive_cursor([src], (refs, ex))
        assert code_of(aclgpu, lambda: e.derive_cursor([src], (refs, ex))) == aclgpu.ERR_RESOURCE_EXHAUSTED
        assert first.info()[1].tolist() == [2] * n_big and chain(first, n_big - 1, 1) == EDGE_SETS[5]
        assert e.count_rows([src], (refs, ex)).tolist() == [2] * n_big  # (a count keeps no rows: the budget does not concern it)
        first.close()
        with e.derive_cursor([src], (refs, ex)) as second:  # after the close: room again
            assert chain(second, 0, 2) == EDGE_SETS[5] and chain(second, n_big - 1, 2) == EDGE_SETS[5]
        # one call whose rows alone exceed the budget
        n_over = BUDGET // row_bytes + 1
        refs2, ex2 = np.zeros((n_over, 2), dtype=np.uint32), np.zeros((n_over, 4), dtype=np.uint32)
        ex2[:, 0] = np.arange(n_over)
        ex2[:, 1] = 1
        assert code_of(aclgpu, lambda: e.derive_cursor([src], (refs2, ex2))) == aclgpu.ERR_RESOURCE_EXHAUSTED


SCHEMA_GROW = """
definition user {}
definition doc { relation viewer: user
 permission view = viewer }
"""


@pytest.mark.parametrize("n0,n_new", [(TILE_IDS, 1), (100, 40)])
def test_unequal_widths(aclgpu, n0, n_new):
    """cursor A is opened while the type has n0 ids; then the user is granted n_new NEW objects, the type grows past a tile (131 072 ids) or past a row's
    padding (128 ids), and cursor B is opened: wider rows, a later revision"""
    with aclgpu.Engine(SCHEMA_GROW) as e:
        u = e.intern("user", "u")
        held = np.array(sorted({0, 31, 32, n0 // 2, n0 - 1}), dtype=np.uint32)
        e.add_edges("doc", "viewer", "user", "", np.array([n0 - 1], dtype=np.uint32), np.array([e.intern("user", "other")], dtype=np.uint32))
        e.add_edges("doc", "viewer", "user", "", held, np.full(held.size, u, dtype=np.uint32))
        assert e.object_count("doc") == n0
        A = e.lookup_cursor("doc", "view", "user", "", [u])
        e.write([(aclgpu.OP_TOUCH, ("doc", f"new{k}", "viewer", "user", "u", "")) for k in range(n_new)])
        new_ids = sorted(e.find("doc", f"new{k}") for k in range(n_new))
        assert new_ids == list(range(n0, n0 + n_new)) and e.object_count("doc") == n0 + n_new
        B = e.lookup_cursor("doc", "view", "user", "", [u])
        rev_a, rev_b = A.info()[0], B.info()[0]
        assert rev_b > rev_a and chain(A, 0, 3) == held.tolist() and chain(B, 0, 3) == held.tolist() + new_ids
        exprs = [([(0, 0), (1, 0)], [], []), ([], [(0, 0), (1, 0)], []), ([(1, 0)], [], [(0, 0)]), ([(0, 0)], [], [(1, 0)])]
        assert code_of(aclgpu, lambda: e.derive_cursor([A, B], exprs)) == aclgpu.ERR_FAILED_PRECONDITION
        assert code_of(aclgpu, lambda: e.count_rows([A, B], exprs)) == aclgpu.ERR_FAILED_PRECONDITION
        counts = e.count_rows([A, B], exprs, any_revision=True)
        with e.derive_cursor([A, B], exprs, any_revision=True) as D:
            rev, ccounts, _flags = D.info()
            assert rev == rev_a  # (the smallest)
            assert ccounts.tolist() == counts.tolist() == [held.size + n_new, held.size, n_new, 0]
            assert chain(D, 0, 4) == held.tolist() + new_ids  # A | B has the new ids
            assert chain(D, 1, 4) == held.tolist()            # A & B does not
            assert chain(D, 2, 4) == new_ids                  # B \ A: exactly the new ids
            assert chain(D, 3, 4) == []
            # the width and the tile count are B's: an id behind A's last word is found, and a page that starts in B's last tile is answered from it
            last = new_ids[-1]
            assert D.page(0, last - 1, 5)[0].tolist() == [last] and D.page(0, last, 5)[0].tolist() == [] and D.page(2, n0 - 1, 1)[0].tolist() == [new_ids[0]]
            # ... and the other way round: sources in the other order, the narrow one last
            with e.derive_cursor([B, A], [([(0, 0)], [], [(1, 0)]), ([], [(1, 0), (0, 0)], [])], any_revision=True) as D2:
                assert D2.info()[0] == rev_a and chain(D2, 0, 2) == new_ids and chain(D2, 1, 2) == held.tolist()
        A.close()
        B.close()


def test_300_expressions_in_one_call(aclgpu):
    rng = np.random.default_rng(20261020)
    n_users, n_docs = 50, 5000
    with aclgpu.Engine(SCHEMA_GROW) as e:
        for u in range(n_users):
            held = np.flatnonzero(rng.random(n_docs) < rng.choice([0.002, 0.05, 0.5, 0.95])).astype(np.uint32)
            held = np.union1d(held, np.array([u, n_docs - 1 - u], dtype=np.uint32)).astype(np.uint32)
            e.add_edges("doc", "viewer", "user", "", held, np.full(held.size, u, dtype=np.uint32))
        e.add_edges("doc", "viewer", "user", "", np.array([n_docs - 1], dtype=np.uint32), np.array([0], dtype=np.uint32))
        assert e.object_count("doc") == n_docs and e.object_count("user") == n_users
        users = list(range(n_users))
        bms, _counts = e.lookup_ids_batch("doc", "view", "user", "", users)
        truth = [bits_of(b, n_docs) for b in bms]
        lists = []
        for _ in range(300):
            k = int(rng.integers(1, 21))
            ops = rng.integers(0, n_users, size=k).tolist()
            n_any = int(rng.integers(0, k + 1))
            n_all = int(rng.integers(0 if n_any else 1, k - n_any + 1))
            lists.append((ops[:n_any], ops[n_any:n_any + n_all], ops[n_any + n_all:]))
        assert {len(a) + len(b) + len(c) for a, b, c in lists} >= {1, 20} and any(not a for a, _b, _c in lists) and any(c for _a, _b, c in lists)
        exprs = [([(0, k) for k in a], [(0, k) for k in b], [(0, k) for k in c]) for a, b, c in lists]
        want = [combine(truth, a, b, c, n_docs) for a, b, c in lists]
        assert sum(int(w.sum()) for w in want) > 10000
        row_bytes = row_bytes_of(n_docs)
        with e.lookup_cursor("doc", "view", "user", "", users) as src:
            before = e.stats()["derive_launches"]
            cur = e.derive_cursor([src], exprs)
            assert e.stats()["derive_launches"] - before == LAUNCHES_PER_DERIVE
            check_derived(e, cur, want)
            cur.close()
            before = e.stats()["derive_launches"]
            with e.derive_cursor([src], exprs[:1]) as one:
                assert e.stats()["derive_launches"] - before == LAUNCHES_PER_DERIVE
                check_derived(e, one, want[:1])
            # count_rows: the same counts, two launches, and nothing taken from the budget -- a derive that fills the budget to the last whole row still
            # succeeds afterwards, and one more row does not
            before = e.stats()["derive_launches"]
            counts = e.count_rows([src], exprs)
            assert e.stats()["derive_launches"] - before == LAUNCHES_PER_DERIVE
            assert counts.tolist() == [int(w.sum()) for w in want]
            n_fill = BUDGET // row_bytes - n_users
            refs = np.zeros((n_fill, 2), dtype=np.uint32)
            refs[:, 1] = np.arange(n_fill) % n_users
            ex = np.zeros((n_fill, 4), dtype=np.uint32)
            ex[:, 0] = np.arange(n_fill)
            ex[:, 1] = 1
            with e.derive_cursor([src], (refs, ex)) as fill:
                assert code_of(aclgpu, lambda: e.derive_cursor([src], exprs[:1])) == aclgpu.ERR_RESOURCE_EXHAUSTED
                assert e.count_rows([src], exprs[:3]).tolist() == counts[:3].tolist()
                assert np.array_equal(fill.info()[1], np.array([int(t.sum()) for t in truth], dtype=np.uint64)[refs[:, 1]])
                assert np.array_equal(fill.page(n_fill - 1, None, n_docs)[0], np.flatnonzero(truth[(n_fill - 1) % n_users]))


def test_subject_direction(aclgpu):
    from aclgpu import workloads
    schema, rels = workloads.SCHEMA_C4, hand_graph()
    co, po = oracles(schema, rels)
    with aclgpu.Engine(schema) as e:
        e.write([(aclgpu.OP_TOUCH, r) for r in rels])
        pods = [f"p{p}" for p in range(6)]
        rids = [e.intern("pod", p) for p in pods]
        for stype, srel in (("user", ""), ("group", "member")):
            names = subject_names(e, stype)

            def holders(p):
                w = {s for s in names if co.check("pod", p, "view", stype, s, srel) == (PERM_HAS, 0)}
                assert w == {s for s in names if po.check("pod", p, "view", stype, s, srel) == HAS}
                return w

            want = [holders("p0") & holders("p1") & holders("p2") & holders("p3"),   # who can view ALL of p0..p3
                    holders("p0") - holders("p5"),                                    # who can view p0 but not p5
                    (holders("p4") | holders("p5")) & holders("p0") - holders("p2")]
            exprs = [([], [(0, 0), (0, 1), (0, 2), (0, 3)], []), ([(0, 0)], [], [(0, 5)]), ([(0, 4), (0, 5)], [(0, 0)], [(0, 2)])]
            with e.subjects_cursor("pod", "view", stype, srel, rids) as src:
                assert not src.info()[2].any()
                counts = e.count_rows([src], exprs)
                with e.derive_cursor([src], exprs) as cur:
                    assert cur.row_type == stype and cur.info()[1].tolist() == counts.tolist() == [len(w) for w in want]
                    for i, w in enumerate(want):
                        for limit in (1, 2, 9):
                            assert {e.object_name(stype, x) for x in chain(cur, i, limit)} == w, (stype, i, limit)
                        ids, nm, _more = cur.page_names(i, None, len(w) + 1)
                        assert set(nm) == w and ids.size == len(w)
            if stype == "user":
                assert want[0] and want[1] != want[0]
    # a row that holds a wildcard is "everyone but ...", not a bitmap: refused where an expression references it, and only there
    rels = [("doc", "open", "viewer", "user", "*", ""), ("doc", "open", "viewer", "user", "u1", ""), ("doc", "mine", "viewer", "user", "u1", ""),
            ("doc", "mine", "viewer", "user", "u2", ""), ("doc", "yours", "viewer", "user", "u2", "")]
    with aclgpu.Engine(SCHEMA_NONMONO) as e:
        e.write([(aclgpu.OP_TOUCH, r) for r in rels])
        rids = [e.intern("doc", d) for d in ("open", "mine", "yours")]
        with e.subjects_cursor("doc", "view", "user", "", rids) as src:
            assert src.info()[2].tolist() == [1, 0, 0]  # ACL_SUBJECTS_WILDCARD on `open`
            for bad in ([([(0, 1)], [], []), ([(0, 1)], [(0, 0)], [])], [([(0, 2)], [], [(0, 0)])], [([(0, 0)], [], [])]):
                assert code_of(aclgpu, lambda: e.derive_cursor([src], bad)) == aclgpu.ERR_FAILED_PRECONDITION
                assert code_of(aclgpu, lambda: e.count_rows([src], bad)) == aclgpu.ERR_FAILED_PRECONDITION
            good = [([], [(0, 1), (0, 2)], []), ([(0, 1)], [], [(0, 2)])]
            assert e.count_rows([src], good).tolist() == [1, 1]
            with e.derive_cursor([src], good) as cur:
                assert [{e.object_name("user", x) for x in chain(cur, i, 2)} for i in range(2)] == [{"u2"}, {"u1"}]


def test_lifetime_and_pinning(aclgpu):
    from aclgpu import workloads
    schema, rels = workloads.SCHEMA_C4, hand_graph()
    co, po = oracles(schema, rels)
    with aclgpu.Engine(schema) as e:
        e.write([(aclgpu.OP_TOUCH, r) for r in rels])
        names = ["ann", "bob", "cy"]
        sids = [e.intern("user", n) for n in names]
        look = {n: co.lookup("pod", "view", "user", n) for n in names}
        assert all(look[n] == po.lookup_resources("pod", "view", "user", n) for n in names)
        want = [look["ann"] | look["bob"], look["ann"] & look["cy"], look["bob"] - look["cy"]]
        src = e.lookup_cursor("pod", "view", "user", "", sids)
        rev0 = src.info()[0]
        cur = e.derive_cursor([src], [([(0, 0), (0, 1)], [], []), ([], [(0, 0), (0, 2)], []), ([(0, 1)], [], [(0, 2)])])
        src.close()  # the derived cursor owns its rows

        def named(c, i):
            return {e.object_name("pod", x) for x in chain(c, i, 2)}

        assert [named(cur, i) for i in range(3)] == want and want[2]
        pages0, info0 = [chain(cur, i, 1) for i in range(3)], cur.info()
        # writes and deletes after the derive do not move it
        ups = [(aclgpu.OP_TOUCH, ("pod", "p9", "viewer", "user", "cy", "")), (aclgpu.OP_DELETE, ("pod", "p2", "viewer", "user", "cy", "")),
               (aclgpu.OP_DELETE, ("pod", "p0", "viewer", "user", "ann", "")), (aclgpu.OP_TOUCH, ("pod", "p9", "viewer", "user", "ann", ""))]
        e.write(ups)
        co.write([(orc.OP_TOUCH if op == aclgpu.OP_TOUCH else orc.OP_DELETE, r) for op, r in ups])
        for op, r in ups:
            po.touch(*r) if op == aclgpu.OP_TOUCH else po.delete(*r)
        for i in range(40):
            e.intern("pod", f"wide{i}")
        e.lookup_ids_batch("pod", "view", "user", "", sids)  # (the snapshot moves on under the cursor)
        assert e.revision > rev0 and [chain(cur, i, 1) for i in range(3)] == pages0
        assert cur.info()[0] == info0[0] == rev0 and cur.info()[1].tolist() == info0[1].tolist()
        # a derived cursor is a legal source -- alone, and next to a fresh open (whose revision and width differ)
        with e.derive_cursor([cur], [([(0, 0)], [], [(0, 1)]), ([], [(0, 0), (0, 1), (0, 0)], [])]) as again:
            assert named(again, 0) == want[0] - want[1] and named(again, 1) == want[0] & want[1] and again.info()[0] == rev0
        with e.lookup_cursor("pod", "view", "user", "", sids) as fresh:
            assert code_of(aclgpu, lambda: e.derive_cursor([cur, fresh], [([(0, 0), (1, 2)], [], [])])) == aclgpu.ERR_FAILED_PRECONDITION
            with e.derive_cursor([cur, fresh], [([(0, 0), (1, 2)], [], []), ([(1, 2)], [], [(0, 0)])], any_revision=True) as mixed:
                now_cy = co.lookup("pod", "view", "user", "cy")
                assert now_cy == po.lookup_resources("pod", "view", "user", "cy")
                assert named(mixed, 0) == want[0] | now_cy and named(mixed, 1) == now_cy - want[0] and "p9" in named(mixed, 1) and mixed.info()[0] == rev0
            # directions and row types do not mix
            with e.subjects_cursor("pod", "view", "user", "", [e.intern("pod", "p0")]) as subj, e.lookup_cursor("namespace", "view", "user", "", sids) as ns:
                for srcs in ([fresh, subj], [subj, fresh], [fresh, ns]):
                    assert code_of(aclgpu, lambda: e.derive_cursor(srcs, [([(0, 0)], [], [(1, 0)])])) == aclgpu.ERR_INVALID_ARGUMENT
                    assert code_of(aclgpu, lambda: e.count_rows(srcs, [([(0, 0)], [], [(1, 0)])])) == aclgpu.ERR_INVALID_ARGUMENT
                # a row beyond a source's rows, and a source that is closed
                assert code_of(aclgpu, lambda: e.derive_cursor([fresh], [([(0, 3)], [], [])])) == aclgpu.ERR_INVALID_ARGUMENT
            gone = e.lookup_cursor("pod", "view", "user", "", sids)
            handle = gone._c
            gone.close()
            closed = aclgpu.LookupCursor(e, handle, "pod", 3)
            assert code_of(aclgpu, lambda: e.derive_cursor([fresh, closed], [([(0, 0)], [], [])])) == aclgpu.ERR_INVALID_ARGUMENT
            closed._c = None
            # no expressions: a valid cursor without rows
            with e.derive_cursor([fresh], []) as empty:
                assert empty.info()[1].size == 0 and empty.pages([]) == []
            assert e.count_rows([fresh], []).size == 0
        # a sharded engine refuses
        e._check(e._L.acl_shard_configure(e._h, 0, 2))
        assert code_of(aclgpu, lambda: e.derive_cursor([cur], [([(0, 0)], [], [])])) == aclgpu.ERR_FAILED_PRECONDITION
        assert code_of(aclgpu, lambda: e.count_rows([cur], [([(0, 0)], [], [])])) == aclgpu.ERR_FAILED_PRECONDITION
        e._check(e._L.acl_shard_configure(e._h, 0, 1))
        assert e.count_rows([cur], [([(0, 0)], [], [])]).tolist() == [len(want[0])]
        # a schema reload expires the derived cursor, as a source too
        e.load_bootstrap(schema)
        for call in (cur.info, lambda: cur.page(0, None, 9), lambda: cur.page_names(0, None, 9), lambda: e.derive_cursor([cur], [([(0, 0)], [], [])]),
                     lambda: e.count_rows([cur], [([(0, 0)], [], [])])):
            assert code_of(aclgpu, call) == aclgpu.ERR_FAILED_PRECONDITION
        cur.close()
    # closing the engine with a derived cursor open
    e = aclgpu.Engine(schema)
    e.write([(aclgpu.OP_TOUCH, r) for r in rels])
    src = e.lookup_cursor("pod", "view", "user", "", [e.intern("user", "ann")])
    d = e.derive_cursor([src], [([(0, 0)], [], [])])
    assert {e.object_name("pod", x) for x in chain(d, 0, 4)} == oracles(schema, rels)[0].lookup("pod", "view", "user", "ann")  # (co has moved on with the writes above)
    e.close()
    d.close()
    src.close()


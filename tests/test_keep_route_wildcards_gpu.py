"""GPU tests of the one-subject reverse route (csrc/engine_keep.cpp keep_by_reverse_walk / keep_by_reverse_walks) on schemas with `T:*`.

The route answers a PostFilter call that names one subject (the KEEP form) and a CheckBulkPermissions of one subject's pairs (the PAIR form) from one reverse
walk plus bit tests -- it is where the engine decides, from the shape of a request, not to ask the Check kernel at all.  Under `viewer: user | user:*` a subject
NO TABLE KNOWS is granted whatever the wildcard's rows grant, so "unknown subject: nothing is allowed, no walk" only holds on a store without a `user:*`
relationship; a subject the table knows only from a `banned` relation holds exactly what the wildcard gives; and `strict = view - banned` must go forward
whoever asks.

Every pair's expected answer is the C oracle's per-pair Check (oracle/orc.py), cross-checked per schema against oracle/pyoracle.py, and the engine's own forward
path (names -> ids -> acl_check_bulk_ids, tests/test_callers_gpu.py _forward_pairs / _forward_keep) tells a route bug from a kernel bug.  The route's counter
(stats()["keep_route_calls"]) is asserted wherever the route's decision is part of the contract, so that "equal answers" cannot mean "the route never ran".
The route is steered by call size (>= 512 pairs) and call order only: the ACL_KEEP_* / ACL_DEPTH_SWEEP knobs are read once per process."""
import contextlib

import numpy as np
import pytest

from oracle import orc, pyoracle
from tests.test_callers_gpu import _forward_keep, _forward_pairs

pytestmark = pytest.mark.gpu

NPOD = 1500  # (below engine_keep.cpp kShortListReach = 4 096: "a short list for a far-reaching subject goes forward" never fires, the counters are deterministic)

SCHEMA_REC = """definition user {}
definition group { relation member: user | user:* | group#member }
definition namespace { relation viewer: user | user:*
 permission view = viewer }
definition pod { relation namespace: namespace
 relation viewer: user | user:* | group#member
 relation banned: user
 permission view = viewer + namespace->view
 permission open = viewer
 permission strict = view - banned }"""

# the same without `group`: no Check can end at the depth limit (Snapshot::slot_deep is false for every slot, as in the reference's bootstrap schema), so the
# pair form takes the route at the first call with no depth sweep
SCHEMA_FLAT = """definition user {}
definition namespace { relation viewer: user | user:*
 permission view = viewer }
definition pod { relation namespace: namespace
 relation viewer: user | user:*
 relation banned: user
 permission view = viewer + namespace->view
 permission open = viewer
 permission strict = view - banned }"""

PERMS = ("view", "open", "strict")
SUBJECTS = ("u1", "u2", "u3", "ghost")  # direct + group grants + bans; known through a namespace only; known ONLY as a banned subject; in no table
GRANTED, DENIED, DEPTH = (2, 0), (1, 0), (0, orc.ERR_DEPTH)  # (on an erring pair the permissionship is 0)

# granted / denied / depth error over p0..p1499 by the C oracle on the recursive graph, recorded when the graph was designed
RECORDED = {("view", "u1"): (781, 573, 146), ("view", "u2"): (915, 468, 117), ("view", "u3"): (623, 701, 176), ("view", "ghost"): (623, 701, 176),
            ("open", "u1"): (543, 765, 192), ("open", "ghost"): (332, 934, 234),
            ("strict", "u1"): (549, 805, 146), ("strict", "u3"): (457, 867, 176), ("strict", "ghost"): (623, 701, 176)}


def _relationships(recursive):
    r = []
    if recursive:
        r += ["group:g1#member@group:g2#member", "group:g2#member@group:g1#member",  # a cycle: pods shared with it answer a depth error unless something grants
              "group:g3#member@user:u1", "group:gw#member@user:*", "group:g4#member@group:g3#member"]
    r += [f"pod:p{i}#namespace@namespace:n{i % 4}" for i in range(NPOD)]
    r += ["namespace:n3#viewer@user:*", "namespace:n2#viewer@user:u2"]
    r += [f"pod:p{i}#viewer@user:*" for i in range(0, NPOD, 7)]
    if recursive:
        r += [f"pod:p{i}#viewer@group:g1#member" for i in range(0, NPOD, 5)]
        r += [f"pod:p{i}#viewer@group:gw#member" for i in range(3, NPOD, 11)]
        r += [f"pod:p{i}#viewer@group:g4#member" for i in range(1, NPOD, 9)]
    r += [f"pod:p{i}#viewer@user:u1" for i in range(2, NPOD, 13)]
    r += [f"pod:p{i}#banned@user:u3" for i in range(0, NPOD, 2)]
    r += [f"pod:p{i}#banned@user:u1" for i in range(0, NPOD, 3)]
    return r


class World:
    """One engine and the two oracles over the same relationships; every write goes to all three, and the expected rows are recomputed after it."""

    def __init__(self, aclgpu, recursive):
        self.recursive = recursive
        self.schema = SCHEMA_REC if recursive else SCHEMA_FLAT
        self.rels = _relationships(recursive)
        self.o = orc.Oracle(self.schema)
        self.py = pyoracle.PyOracle(self.schema)
        self.e = aclgpu.Engine(self.schema)
        self._rows = {}
        self.write(orc.OP_TOUCH, self.rels)

    def write(self, op, rels):
        for b in range(0, len(rels), 1000):  # (at most 1 000 updates per write)
            ups = [(op, r) for r in rels[b:b + 1000]]
            self.o.write(ups)
            self.e.write(ups)
        for r in rels:
            (self.py.touch if op == orc.OP_TOUCH else self.py.delete)(*orc.parse_rel(r))
        self._rows.clear()

    def answer(self, perm, subject, pod):
        """the oracle's Check of one pair -> (permissionship, error); every (permission, subject) row over p0..p1499 is computed once per state of the store"""
        row = self._rows.get((perm, subject))
        if row is None:
            row = self._rows[perm, subject] = {f"p{i}": self.o.check("pod", f"p{i}", perm, "user", subject) for i in range(NPOD)}
        a = row.get(pod)
        if a is None:  # (a name the pod table does not hold)
            a = row[pod] = self.o.check("pod", pod, perm, "user", subject)
        return a

    def counts(self, perm, subject):
        row = [self.answer(perm, subject, f"p{i}") for i in range(NPOD)]
        assert set(row) <= {GRANTED, DENIED, DEPTH}, (perm, subject)
        return tuple(sum(a == w for a in row) for w in (GRANTED, DENIED, DEPTH))

    def pyoracle_agrees(self, perm, subject):
        as_pair = {pyoracle.HAS: GRANTED, pyoracle.NO: DENIED, pyoracle.ERR: DEPTH}
        return all(as_pair[self.py.check("pod", f"p{i}", perm, "user", subject)] == self.answer(perm, subject, f"p{i}") for i in range(NPOD))

    def calls(self):
        return self.e.stats()["keep_route_calls"]

    def close(self):
        self.e.close()
        self.o.close()


@contextlib.contextmanager
def _world(aclgpu, recursive):
    w = World(aclgpu, recursive)
    try:
        yield w
    finally:
        w.close()


@pytest.fixture(scope="module")
def aclgpu(aclgpu_lib):
    import aclgpu as m
    return m


@pytest.fixture(scope="module", params=["recursive", "flat"])
def world(request, aclgpu):
    """the engine the keep-form tests share (they write nothing; the keep form needs no depth sweep, so no test depends on another's calls)"""
    with _world(aclgpu, request.param == "recursive") as w:
        yield w


def _pods(rng, k):  # k resource names: random pods (repeats included), every 13th a name the pod table does not hold
    return [f"p{int(p)}" if j % 13 else f"nowhere-{j}" for j, p in enumerate(rng.integers(0, NPOD, size=k))]


def _pairs(pods, perm, subject):
    return [("pod", p, perm, "user", subject, "") for p in pods]


def _want_keep(w, items, off):  # an item is kept if and only if all its pairs are (2, 0); one without pairs is kept (postfilter.go:145-178)
    return np.array([all(w.answer(items[j][2], items[j][4], items[j][1]) == GRANTED for j in range(off[i], off[i + 1])) for i in range(len(off) - 1)], dtype=bool)


def _route_moves(w, perm, subject, walks=1):
    """by how much keep_route_calls must move for one call of a known / unknown subject, or None where the contract leaves it open"""
    if perm == "strict":
        return 0  # a non-monotone permission goes forward, whoever asks
    if subject in w.unknown:
        return None if w.wildcards else walks  # under a `user:*` relationship the route may decline or walk: the answers decide; without one it answers itself
    return walks


def _check_keep(w, items, off, perm, subject, forms=("views",), walks=1):
    want = _want_keep(w, items, off)
    assert np.array_equal(_forward_keep(w.e, items, off), want), ("the forward path differs from the oracle", perm, subject)
    for form in forms:
        before = w.calls()
        if form == "views":
            got = w.e.check_bulk_keep_views(w.e.make_check_views(items), off)
        elif form == "packed":
            got = w.e.check_bulk_keep_packed(w.e.make_check_packed(items), off)
        else:
            got = w.e.check_bulk_keep(items, off)
        moved = w.calls() - before
        got = np.asarray(got).astype(bool)
        wrong = np.flatnonzero(got != want)
        assert wrong.size == 0, (f"{form}: {wrong.size} of {want.size} items differ from the oracle ({int(want.sum())} kept by the oracle, {int(got.sum())} by the call; "
                                 f"the forward path agrees with the oracle), first at item {int(wrong[0])}", perm, subject, "route calls", moved)
        expect = _route_moves(w, perm, subject, walks)
        assert expect is None or moved == expect, (form, perm, subject, moved)
    return want


def _prepare(w):
    """what the store of a freshly written world holds, and what the oracles say of it -- asserted BEFORE the engine is looked at: an all-NO answer cannot pass"""
    w.unknown, w.wildcards = {"ghost", "phantom"}, True
    for perm in PERMS:
        for s in SUBJECTS:
            g, d, x = w.counts(perm, s)
            assert g >= 0.05 * NPOD and d >= 0.05 * NPOD and (x >= 0.05 * NPOD if w.recursive else x == 0), (perm, s, g, d, x)
            if w.recursive and (perm, s) in RECORDED:
                assert (g, d, x) == RECORDED[perm, s], (perm, s)
    assert w.counts("view", "ghost")[0] > 0 and w.counts("open", "ghost")[0] > 0 and w.counts("strict", "ghost")[0] > 0  # granted, and only through `user:*`
    assert w.e.find("user", "ghost") is None and w.e.find("user", "u3") is not None and w.e.find("user", "*") is not None


def test_expected_values_meet_every_outcome_and_both_oracles_agree(world):
    """The reference values themselves, before any call of the route: per (subject, permission) at least 5 % of the 1 500 pods are granted, 5 % denied and -- on the
    recursive graph -- 5 % a depth error; the unknown subject is granted somewhere; the counts are the ones recorded with the graph; oracle/pyoracle.py gives every
    pair of `ghost` (all three permissions) and of `u1` on `strict` the same answer as the C oracle; a pod behind the group cycle that also carries a wildcard is
    granted (HAS_PERMISSION wins), the next one behind the cycle without a wildcard is the depth error."""
    w = world
    _prepare(w)
    for perm in PERMS:
        assert w.pyoracle_agrees(perm, "ghost"), perm
    assert w.pyoracle_agrees("strict", "u1")
    if w.recursive:
        assert w.answer("open", "ghost", "p35") == GRANTED and w.answer("open", "ghost", "p5") == DEPTH  # (p35: viewer@group:g1#member AND viewer@user:*)
    # and the forward path: one id call per (subject, permission) over every pod
    for perm in PERMS:
        for s in SUBJECTS:
            items = _pairs([f"p{i}" for i in range(NPOD)], perm, s)
            fp, fe = _forward_pairs(w.e, items)
            assert list(zip(fp.tolist(), fe.tolist())) == [w.answer(perm, s, it[1]) for it in items], ("the forward path differs from the oracle", perm, s)


def test_keep_600_items_on_the_callers_thread_by_all_three_entry_points(world):
    """Keep form, one pair per item, 600 items (below kSpreadMin: walk, then pass, on the caller's thread), through acl_check_bulk_keep_v, _packed and the
    NUL-terminated form, for every subject and permission.  Known subjects on `view` / `open` take the route (+1 per call: the route runs under wildcards); `strict`
    leaves the counter alone; `ghost` must be kept wherever `user:*` grants it."""
    w = world
    _prepare(w)
    rng = np.random.default_rng(600)
    for s in SUBJECTS:
        for perm in PERMS:
            items = _pairs(_pods(rng, 600), perm, s)
            want = _check_keep(w, items, np.arange(601, dtype=np.uint32), perm, s, forms=("views", "packed", "cstr"))
            assert 0 < want.sum() < 600, (perm, s)


def test_keep_2100_and_11000_items_through_the_pool_many_and_few_allowed(world):
    """Keep form through the interning pool (from kSpreadMin = 2 048 items on), pods repeated.  At 2 100 items every subject's allowed count (>= 215 pods: the
    wildcard's own) is above max(kFewFloor, n / kFewShare) = 65, so every name goes to the table (MANY).  The tag path (FEW) needs allowed <= n / 32: `u2` and `u3`
    hold on `open` only what `user:*` gives (332 pods on the recursive graph, 215 on the flat one), which is FEW from 10 624 pairs on -- one call of 11 000 items
    each takes it; `u1` on `view` stays MANY there."""
    w = world
    _prepare(w)
    rng = np.random.default_rng(2100)
    for s in SUBJECTS:
        for perm in PERMS:
            items = _pairs(_pods(rng, 2100), perm, s)
            want = _check_keep(w, items, np.arange(2101, dtype=np.uint32), perm, s)
            assert 0 < want.sum() < 2100, (perm, s)
    for s, perm in (("u2", "open"), ("u3", "open"), ("u1", "view"), ("ghost", "open")):
        assert (w.counts(perm, s)[0] <= 11000 // 32) == (perm == "open")
        items = _pairs(_pods(rng, 11000), perm, s)
        _check_keep(w, items, np.arange(11001, dtype=np.uint32), perm, s)


def test_keep_ragged_items_of_0_to_3_pairs(world):
    """Keep form, 1 500 items of 0..3 pairs each: an item is kept when ALL its pairs are granted, one without pairs is kept."""
    w = world
    _prepare(w)
    rng = np.random.default_rng(1500)
    for s in SUBJECTS:
        for perm in PERMS:
            nper = rng.integers(0, 4, size=1500)
            off = np.concatenate([[0], np.cumsum(nper)]).astype(np.uint32)
            items = _pairs(_pods(rng, int(off[-1])), perm, s)
            want = _check_keep(w, items, off, perm, s)
            assert want[nper == 0].all() and not want[nper > 0].all() and want[nper > 0].any(), (perm, s)


def test_keep_k_items_times_two_templates(world):
    """K x F (keep_by_reverse_walks): 600 items x the templates (`view`, `open`) through acl_check_bulk_keep_v -- one walk per template for a known subject (+2),
    the AND of both masks; (`view`, `strict`): the non-monotone template sends the whole call forward."""
    w = world
    _prepare(w)
    rng = np.random.default_rng(1200)
    off = np.arange(0, 1201, 2, dtype=np.uint32)
    for s in SUBJECTS:
        pods = _pods(rng, 600)
        items = [("pod", p, perm, "user", s, "") for p in pods for perm in ("view", "open")]
        want = _check_keep(w, items, off, "view+open", s, walks=2)
        assert 0 < want.sum() < 600, s
        items = [("pod", p, perm, "user", s, "") for p in pods for perm in ("view", "strict")]
        _check_keep(w, items, off, "strict", s)


def test_a_wildcard_as_the_subject_of_a_keep_call_is_refused(world):
    """`*` as a subject id of a Check is refused by validation on both routes: the keep call fails with InvalidArgument, the route's counter stands still."""
    import aclgpu
    w = world
    items = _pairs([f"p{i}" for i in range(600)], "view", "*")
    before = w.calls()
    with pytest.raises(aclgpu.AclError) as ei:
        w.e.check_bulk_keep_views(w.e.make_check_views(items), np.arange(601, dtype=np.uint32))
    assert ei.value.code == aclgpu.ERR_INVALID_ARGUMENT and w.calls() == before


def _pair_calls(w, items):
    return (("views", lambda: w.e.check_bulk_views(w.e.make_check_views(items))), ("packed", lambda: w.e.check_bulk_packed(w.e.make_check_packed(items))),
            ("prepared", lambda: w.e.check_bulk_prepared(w.e.make_check_strings_named(items))))


def _check_pairs(w, items, perm, subject, calls):
    """every pair's permissionship AND error code against the oracle -> how far keep_route_calls moved over `calls`"""
    want = [w.answer(perm, subject, it[1]) for it in items]
    fp, fe = _forward_pairs(w.e, items)
    assert list(zip(fp.tolist(), fe.tolist())) == want, ("the forward path differs from the oracle", perm, subject)
    before = w.calls()
    for form, call in calls:
        p, er = call()
        got = list(zip(p.tolist(), er.tolist()))
        wrong = [j for j in range(len(want)) if got[j] != want[j]]
        assert not wrong, (f"{form}: {len(wrong)} of {len(want)} pairs differ from the oracle (the forward path agrees with it), first {items[wrong[0]][1]}: "
                           f"{got[wrong[0]]} for {want[wrong[0]]}", perm, subject, "route calls", w.calls() - before)
    return w.calls() - before


def test_pair_form_on_the_flat_schema_takes_the_route_at_the_first_call(aclgpu):
    """CheckBulkPermissions of one subject's 1 500 pairs (acl_check_bulk_v, _packed, acl_check_bulk) where no Check can end at the depth limit: the route answers the
    very first call -- +1 per call for a known subject on `view` / `open` under wildcards, nothing on `strict`; `ghost` is HAS_PERMISSION wherever `user:*` is."""
    with _world(aclgpu, False) as w:
        _prepare(w)
        rng = np.random.default_rng(15)
        for s in SUBJECTS:
            for perm in PERMS:
                items = _pairs(_pods(rng, 1500), perm, s)
                moved = _check_pairs(w, items, perm, s, _pair_calls(w, items))
                expect = _route_moves(w, perm, s, walks=3)
                assert expect is None or moved == expect, (perm, s, moved)
        assert w.e.stats()["depth_sweeps"] == 0


def test_pair_form_on_the_recursive_schema_answers_depth_errors_from_the_deep_bitmap(aclgpu):
    """The pair form where `group#member` is recursive and two groups contain each other: per permission the first call at the snapshot goes forward and leaves a
    note, the second sweeps the type (depth_sweeps + 1) and walks, the third walks; the depth errors are then answered per pair from the deep objects' bitmap -- for
    `ghost` too -- and a pod behind the cycle that carries a wildcard is (2, 0), not an error.  Structure of tests/test_callers_gpu.py
    test_check_bulk_of_one_subject_behind_a_cycle_of_groups_carries_the_depth_errors."""
    with _world(aclgpu, True) as w:
        _prepare(w)
        items = {(perm, s): _pairs([f"p{i}" for i in range(NPOD)], perm, s) for perm in PERMS for s in SUBJECTS}
        assert w.answer("view", "ghost", "p35") == GRANTED and w.answer("open", "u3", "p35") == GRANTED and w.answer("open", "u3", "p5") == DEPTH
        for perm in ("view", "open"):
            st0 = w.e.stats()
            moved = _check_pairs(w, items[perm, "u1"], perm, "u1", _pair_calls(w, items[perm, "u1"]))
            st1 = w.e.stats()
            assert moved == 2 and st1["depth_sweeps"] == st0["depth_sweeps"] + 1, (perm, moved)  # forward + note; sweep + walk; walk
            for s in ("u2", "u3"):  # the snapshot is known: every call walks, the errors from the bitmap
                assert _check_pairs(w, items[perm, s], perm, s, _pair_calls(w, items[perm, s])) == 3, (perm, s)
            _check_pairs(w, items[perm, "ghost"], perm, "ghost", _pair_calls(w, items[perm, "ghost"]))
            assert w.e.stats()["depth_sweeps"] == st1["depth_sweeps"]
        for s in SUBJECTS:
            assert _check_pairs(w, items["strict", s], "strict", s, _pair_calls(w, items["strict", s])) == 0, s
        # the keep call drops an item on either answer and walks from the start
        for s in ("u1", "ghost"):
            _check_keep(w, items["open", s], np.arange(NPOD + 1, dtype=np.uint32), "open", s)


@pytest.mark.parametrize("recursive", [True, False], ids=["recursive", "flat"])
def test_the_unknown_subject_becomes_known_and_the_wildcards_leave(aclgpu, recursive):
    """The guard follows the STORE, not the name table.  `pod:p4#viewer@user:ghost` is written: `ghost` is a known subject now and takes the route (+1 per call on
    `view` / `open`), holding the wildcard's pods and p4.  Then every `user:*` relationship is deleted -- the `*` object stays in the user table with no relationship
    left: every subject again, and `phantom`, whom no table knows, is answered by the route itself again (+1, no walk: nothing is allowed but what is behind no
    cycle either), as on any wildcard-free store.  Expected values from oracles that received the same writes."""
    with _world(aclgpu, recursive) as w:
        _prepare(w)
        rng = np.random.default_rng(4)
        off = np.arange(601, dtype=np.uint32)
        everybody = [f"p{i}" for i in range(NPOD)]

        def both_forms(s, perm):
            _check_keep(w, _pairs(["p4"] + _pods(rng, 599), perm, s), off, perm, s, forms=("views", "packed"))
            items = _pairs(everybody, perm, s)
            moved = _check_pairs(w, items, perm, s, _pair_calls(w, items))  # (on the recursive schema: forward, sweep + walk, walk -- whatever the last write left)
            expect = _route_moves(w, perm, s, walks=3)
            assert w.recursive or expect is None or moved == expect, (perm, s, moved)

        assert w.answer("open", "ghost", "p4") == DENIED
        both_forms("ghost", "open")
        w.write(orc.OP_TOUCH, ["pod:p4#viewer@user:ghost"])
        w.unknown = {"phantom"}
        assert w.e.find("user", "ghost") is not None and w.answer("open", "ghost", "p4") == GRANTED and w.answer("open", "phantom", "p4") == DENIED
        for perm in PERMS:
            both_forms("ghost", perm)
        both_forms("phantom", "view")
        stars = [r for r in w.rels if r.endswith("@user:*")]
        assert len(stars) == len(range(0, NPOD, 7)) + (2 if recursive else 1)
        w.write(orc.OP_DELETE, stars)
        w.wildcards = False
        assert w.e.find("user", "*") is not None and not any(w.e.read(rtype=t, stype="user", sid="*") for t in ("pod", "namespace") + (("group",) if recursive else ()))
        assert w.counts("view", "phantom")[0] == 0 and w.counts("open", "ghost")[0] == 1 and w.counts("view", "u1")[0] > 0.05 * NPOD
        assert w.pyoracle_agrees("view", "phantom") and w.pyoracle_agrees("strict", "u1")
        for s in SUBJECTS + ("phantom",):
            for perm in PERMS:
                both_forms(s, perm)


def test_a_clock_set_back_closes_a_ring_of_groups_behind_the_depth_sweep(aclgpu):
    """"None is deep" (engine_keep.cpp no_object_is_deep) must not outlive a clock that is set back.  A ring of three groups whose closing nesting expires at T,
    200 of 600 pods viewed through the ring.  Past T the ring is open: the one-user CheckBulkPermissions goes forward, then sweeps (none deep) and takes the reverse
    route.  Then the clock is set back below T WITH NO WRITE: the expired, not yet collected nesting is alive again and closes the ring, so the pods behind it answer
    the depth error for whoever is not found first -- by both oracles.  The same call and the keep call must say so too: permissionship, error and keep byte of every
    pair.  (The sweep is reached by call order, as everywhere in this file: the ACL_DEPTH_SWEEP knob is read once per process.)"""
    schema = """definition user {}
definition group { relation member: user | group#member with expiration }
definition pod { relation viewer: user | group#member
 permission view = viewer }"""
    t_exp = 1_700_000_100
    rels = ["group:r0#member@group:r1#member", "group:r1#member@group:r2#member", "group:r1#member@user:u1", "group:g3#member@user:u2"]
    rels += [f"pod:p{i}#viewer@group:r0#member" for i in range(0, 600, 3)] + [f"pod:p{i}#viewer@user:u2" for i in range(1, 600, 3)]
    rels += [f"pod:p{i}#viewer@group:g3#member" for i in range(2, 600, 6)]
    closing = "group:r2#member@group:r0#member"
    o, py = orc.Oracle(schema), pyoracle.PyOracle(schema)
    with aclgpu.Engine(schema) as e:
        def at(now):
            e.set_now(now)
            o.set_now(now)
            py.now = now

        def expected(u):
            items = [("pod", f"p{i}", "view", "user", u, "") for i in range(600)]
            want = [tuple(o.check(*q)) for q in items]
            as_pair = {pyoracle.HAS: GRANTED, pyoracle.NO: DENIED, pyoracle.ERR: DEPTH}
            assert [as_pair[py.check(*q)] for q in items] == want, ("the two oracles differ", u)
            return items, want

        def same(u, calls):
            items, want = expected(u)
            for k in range(calls):
                p, er = e.check_bulk(items)
                got = list(zip(p, er))
                wrong = [i for i in range(600) if got[i] != want[i]]
                assert not wrong, (u, f"call {k}: {len(wrong)} of 600 pairs differ from the oracles, first {items[wrong[0]][1]}: {got[wrong[0]]} for {want[wrong[0]]}", e.stats()["keep_route_calls"])
            keep = np.asarray(e.check_bulk_keep(items, list(range(601)))).astype(bool)
            assert keep.tolist() == [w_ == GRANTED for w_ in want], u
            return want

        at(t_exp - 100)
        ups = [(orc.OP_TOUCH, r) for r in rels] + [(orc.OP_TOUCH, closing, t_exp)]
        o.write(ups)
        e.write(ups)
        for r in rels:
            py.touch(*orc.parse_rel(r))
        py.touch(*orc.parse_rel(closing), expires=t_exp)
        assert sum(w_ == DEPTH for w_ in expected("u2")[1]) == 200  # (the ring is closed: what the clock set back must bring back)
        # ---- past T: the ring is open, nothing is deep; forward + note, sweep + walk, walk
        at(t_exp + 10)
        st0 = e.stats()
        for u in ("u2", "stranger"):
            want = same(u, 3)
            assert DEPTH not in want and (u == "stranger" or 250 < sum(w_ == GRANTED for w_ in want) < 600)
        st1 = e.stats()
        assert st1["depth_sweeps"] > st0["depth_sweeps"] and st1["keep_route_calls"] > st0["keep_route_calls"], (st0, st1)
        # ---- back below T, no write: the closing nesting is alive again
        at(t_exp - 50)
        for u in ("u2", "stranger", "u1"):
            want = same(u, 2)
            assert sum(w_ == DEPTH for w_ in want) == (0 if u == "u1" else 200), u  # (u1 is IN the ring: found before the limit)
        # ---- and forward again: open, shallow
        at(t_exp + 20)
        for u in ("u2", "stranger"):
            assert DEPTH not in same(u, 2)
    o.close()

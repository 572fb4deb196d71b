"""Watch sets on the GPU (csrc/engine_watchset.cpp, kernels.hip k_rows_diff_*): every poll's records against the set differences of the
oracles' LookupResources -- the C oracle and the Python oracle on the same writes, never the engine's own lookups alone.

A record is (watcher, resource id, gained); a poll's records are ordered by (watcher, resource id), so whole arrays are compared."""
import numpy as np
import pytest

from oracle import orc
from oracle.pyoracle import LookupFailed, PyOracle
from tests.watch_records import expected_records, records_of

pytestmark = pytest.mark.gpu

OP_TOUCH, OP_DELETE = 2, 3


@pytest.fixture(scope="module")
def aclgpu(aclgpu_lib):
    import aclgpu as m
    return m


class World:
    """One engine, the C oracle and the Python oracle under the same writes; `held` is what every watcher held at its last poll."""

    def __init__(self, aclgpu, schema, rt="pod", perm="view", st="user", **kw):
        self.e = aclgpu.Engine(schema, device=kw.pop("device", 0), **kw)
        self.o = orc.Oracle(schema)
        self.p = PyOracle(schema)
        self.rt, self.perm, self.st = rt, perm, st
        self.ws = self.e.watch_set(rt, perm, st)
        self.subject, self.held = {}, {}

    def close(self):
        self.ws.close()
        self.e.close()

    def write(self, ups):
        for k in range(0, len(ups), 1000):  # (WriteRelationships takes 1000 updates at most)
            self.e.write(ups[k:k + 1000])
            self.o.write(ups[k:k + 1000])
        for u in ups:
            if u[0] == OP_DELETE:
                self.p.delete(*u[1])
            else:
                self.p.touch(*u[1], expires=u[2] if len(u) > 2 else 0)

    def set_now(self, t):
        self.e.set_now(t)
        self.o.set_now(t)
        self.p.now = t

    def lookup(self, sid, py=True):
        a = self.o.lookup(self.rt, self.perm, self.st, sid)
        if py:
            assert a == self.p.lookup_resources(self.rt, self.perm, self.st, sid), sid  # the two oracles agree
        return a

    def add(self, sid, from_now=False):
        w = self.ws.add(sid, from_now=from_now)
        self.subject[w] = sid
        self.held[w] = None if from_now else set()  # None: whatever it holds at the next poll
        return w

    def remove(self, w):
        self.ws.remove(w)
        del self.subject[w], self.held[w]

    def expected(self, py=True):
        """the records the next poll must return, and what every watcher holds then"""
        after = {w: self.lookup(self.subject[w], py) for w in sorted(self.subject)}
        return expected_records(self.held, after, lambda n: self.e.find(self.rt, n)), after

    def poll_and_compare(self, tag=None, py=True):
        want, after = self.expected(py)
        rev, recs = self.ws.poll()
        got = records_of(recs)
        assert got == want, tag
        assert rev == self.e.revision and not recs["reserved"].any()
        self.held = after
        return got

    def rows_match(self):
        for w, sid in self.subject.items():
            want = sorted(self.e.find(self.rt, n) for n in self.held[w])
            assert self.ws.row(w).tolist() == want, (w, sid)


SCHEMA_NESTED = """
definition user {}
definition group {
  relation member: user | group#member
}
definition namespace {
  relation viewer: group#member
  permission view = viewer
}
definition pod {
  relation namespace: namespace
  permission view = namespace->view
}
"""


def test_transitive_change_is_reported_where_the_recheck_hears_nothing(aclgpu):
    """pod -> namespace -> group#member -> group#member -> user, 70 pods (a row crosses a 32-bit word and a 64-bit pair), 3 watchers with a FROM_NOW
    baseline.  ONE group#member@user relationship: the watcher gains exactly Oracle.lookup(after) - Oracle.lookup(before); acl_watch_recheck for
    type pod reports no update at all (the gap this closes); the membership deleted: everything comes back as lost."""
    w = World(aclgpu, SCHEMA_NESTED)
    try:
        ups = []
        for n in range(3):
            ups += [(OP_TOUCH, ("namespace", f"ns{n}", "viewer", "group", f"top{n}", "member")), (OP_TOUCH, ("group", f"top{n}", "member", "group", f"mid{n}", "member"))]
        ups += [(OP_TOUCH, ("pod", f"ns{i % 3}/p{i}", "namespace", "namespace", f"ns{i % 3}", "")) for i in range(70)]
        ups += [(OP_TOUCH, ("group", "mid0", "member", "user", "ua", "")), (OP_TOUCH, ("group", "mid2", "member", "user", "ub", ""))]
        w.write(ups)
        wa, wb, wc = w.add("ua", True), w.add("ub", True), w.add("uc", True)
        assert w.poll_and_compare("baseline") == []
        w.rows_match()
        assert len(w.held[wa]) == 24 and len(w.held[wb]) == 23 and not w.held[wc]
        cursor = w.e.revision
        w.write([(OP_TOUCH, ("group", "mid1", "member", "user", "ua", ""))])
        got = w.poll_and_compare("membership")
        assert len(got) == 23 and all(x[0] == wa and x[2] == 1 for x in got)  # ns1's pods, for ua alone
        assert max(x[1] for x in got) >= 64 and min(x[1] for x in got) < 32
        updates, _cur = w.e.watch_recheck(cursor, "pod", "view", "user", "ua")
        assert updates == []  # the reference-shaped watch path hears nothing: no update of type pod exists
        w.rows_match()
        w.write([(OP_DELETE, ("group", "mid1", "member", "user", "ua", ""))])
        back = w.poll_and_compare("membership deleted")
        assert [(a, b) for a, b, _g in back] == [(a, b) for a, b, _g in got] and all(g == 0 for _a, _b, g in back)
        w.rows_match()
        assert w.ws.stats() == {"polls": 3, "walks": 3, "changes": 46}
    finally:
        w.close()


SCHEMA_STREAM = """
definition user {}
definition group {
  relation member: user | group#member
}
definition namespace {
  relation viewer: user | user:* | group#member
  permission view = viewer
}
definition pod {
  relation namespace: namespace
  relation viewer: user | group#member
  permission view = viewer + namespace->view
}
"""


def test_seeded_random_stream(aclgpu):
    """40 steps of touches and deletes over an arrow, userset subjects and a `user:*` grant; 8 watchers, one added mid-stream without FROM_NOW (its
    first poll reports all it holds) and one removed; a poll after every step equals the oracles' set differences; at the end every row equals the
    oracles' lookup."""
    rng = np.random.default_rng(20261018)
    w = World(aclgpu, SCHEMA_STREAM)
    try:
        pods = [f"n{i % 3}/p{i}" for i in range(40)]
        w.write([(OP_TOUCH, ("pod", p, "namespace", "namespace", p.split("/")[0], "")) for p in pods])
        users, groups = [f"u{i}" for i in range(9)], [f"g{i}" for i in range(4)]
        for i in range(7):
            w.add(users[i], from_now=bool(i % 2))
        live, total = [], 0
        for step in range(40):
            if step == 15:
                w.add(users[7])  # from the empty row
            if step == 25:
                w.remove(2)
            if live and rng.random() < 0.35:
                ups = [(OP_DELETE, live.pop(int(rng.integers(len(live)))))]
            else:
                kind = int(rng.integers(7))
                u, g, p, n = users[rng.integers(9)], int(rng.integers(4)), pods[rng.integers(40)], f"n{rng.integers(3)}"
                rel = [("pod", p, "viewer", "user", u, ""), ("pod", p, "viewer", "group", groups[g], "member"), ("group", groups[g], "member", "user", u, ""),
                       ("group", groups[g], "member", "group", groups[(g + 1) % 4] if g < 3 else groups[0], "member"), ("namespace", n, "viewer", "user", u, ""),
                       ("namespace", n, "viewer", "user", "*", ""), ("namespace", n, "viewer", "group", groups[g], "member")][kind]
                if kind == 3 and g == 3:
                    rel = ("group", "g3", "member", "user", u, "")  # (nesting only upwards g0 <- g1 <- g2 <- g3: no cycles in this stream)
                ups = [(OP_TOUCH, rel)]
                if rel not in live:
                    live.append(rel)
            w.write(ups)
            total += len(w.poll_and_compare((step, ups)))
        assert total > 20 and len(w.subject) == 7
        w.rows_match()
        assert any(w.held[x] for x in w.held)
    finally:
        w.close()


SCHEMA_NS = """
definition user {}
definition namespace {
  relation viewer: user | user:*
  permission view = viewer
}
definition pod {
  relation namespace: namespace
  permission view = namespace->view
}
"""


def test_width_growth(aclgpu):
    """A baseline taken with 31 pods (one word); then 2 100 pods and a namespace grant: the gained ids beyond the old rows' width are reported, and nothing else."""
    w = World(aclgpu, SCHEMA_NS)
    try:
        w.write([(OP_TOUCH, ("pod", f"a/p{i}", "namespace", "namespace", "a", "")) for i in range(31)] + [(OP_TOUCH, ("namespace", "a", "viewer", "user", "u0", ""))])
        w0, w1 = w.add("u0"), w.add("u1")
        assert len(w.poll_and_compare("baseline", py=False)) == 31
        w.write([(OP_TOUCH, ("pod", f"b/p{i}", "namespace", "namespace", "b", "")) for i in range(2100)] + [(OP_TOUCH, ("namespace", "b", "viewer", "user", "u1", ""))])
        got = w.poll_and_compare("grown", py=False)
        assert len(got) == 2100 and all(x[0] == w1 and x[2] == 1 and x[1] >= 31 for x in got) and w.e.object_count("pod") == 2131
        w.rows_match()
        assert w.poll_and_compare("again", py=False) == []
    finally:
        w.close()


def test_dense_flip(aclgpu):
    """A `user:*` grant on the namespace flips every bit of every watcher's row at once (every lane emits 32 records per word); then back."""
    w = World(aclgpu, SCHEMA_NS)
    try:
        w.write([(OP_TOUCH, ("pod", f"a/p{i}", "namespace", "namespace", "a", "")) for i in range(300)])
        for u in ("u0", "u1", "u2"):
            w.add(u)
        assert w.poll_and_compare("empty", py=False) == []
        w.write([(OP_TOUCH, ("namespace", "a", "viewer", "user", "*", ""))])
        got = w.poll_and_compare("flip", py=False)
        assert got == [(x, i, 1) for x in range(3) for i in range(300)]
        w.write([(OP_DELETE, ("namespace", "a", "viewer", "user", "*", ""))])
        assert w.poll_and_compare("flip back", py=False) == [(x, i, 0) for x in range(3) for i in range(300)]
        w.rows_match()
    finally:
        w.close()


SCHEMA_LIVE = """
definition user {}
definition doc {
  relation viewer: user with expiration
  permission view = viewer
}
"""


def test_expiry_without_a_write(aclgpu):
    """A grant with expires_at: after the clock passes it -- and no write at all -- a poll reports it lost."""
    w = World(aclgpu, SCHEMA_LIVE, rt="doc")
    try:
        now = 1_800_000_000
        w.set_now(now)
        w.write([(OP_TOUCH, ("doc", "d0", "viewer", "user", "u0", "")), (OP_TOUCH, ("doc", "d1", "viewer", "user", "u0", ""), now + 100)])
        w0 = w.add("u0")
        assert w.poll_and_compare("both") == [(w0, 0, 1), (w0, 1, 1)]
        w.set_now(now + 101)
        assert w.poll_and_compare("expired") == [(w0, 1, 0)]
        w.rows_match()
    finally:
        w.close()


def test_noop_poll_walks_nothing(aclgpu):
    w = World(aclgpu, SCHEMA_NS)
    try:
        w.write([(OP_TOUCH, ("pod", "a/p0", "namespace", "namespace", "a", "")), (OP_TOUCH, ("namespace", "a", "viewer", "user", "u0", ""))])
        w.add("u0")
        assert len(w.poll_and_compare("first")) == 1
        before = w.ws.stats()
        rev, recs = w.ws.poll()
        assert recs.size == 0 and rev == w.e.revision
        after = w.ws.stats()
        assert after["walks"] == before["walks"] and after["polls"] == before["polls"] + 1 and after["changes"] == before["changes"]
    finally:
        w.close()


SCHEMA_BAN = """
definition user {}
definition group {
  relation member: user | group#member
}
definition pod {
  relation viewer: user | group#member
  relation banned: user | group#member
  permission view = viewer - banned
}
"""


def test_exclusion_and_atomic_failure(aclgpu):
    """view = viewer - banned: banning a user reports that user's pods lost.  A cycle of groups behind a candidate's `banned`: its confirming Check runs
    into the depth limit, the poll fails with ERR_DEPTH and row() still shows the baseline; the cycle deleted: the next poll reports exactly the oracles'
    difference against that baseline (a change written while the poll was failing included)."""
    w = World(aclgpu, SCHEMA_BAN)
    try:
        w.write([(OP_TOUCH, ("pod", f"p{i}", "viewer", "user", f"u{i % 2}", "")) for i in range(40)])
        w0, w1 = w.add("u0"), w.add("u1")
        assert len(w.poll_and_compare("baseline")) == 40
        w.write([(OP_TOUCH, ("pod", f"p{i}", "banned", "user", "u0", "")) for i in (0, 2, 36)])
        assert w.poll_and_compare("banned") == [(w0, 0, 0), (w0, 2, 0), (w0, 36, 0)]
        w.rows_match()
        cycle = [("pod", "p4", "banned", "group", "ga", "member"), ("group", "ga", "member", "group", "gb", "member"), ("group", "gb", "member", "group", "ga", "member")]
        w.write([(OP_TOUCH, r) for r in cycle] + [(OP_TOUCH, ("pod", "p41", "viewer", "user", "u1", ""))])
        with pytest.raises(LookupFailed):
            w.p.lookup_resources("pod", "view", "user", "u0")
        with pytest.raises(aclgpu.AclError) as ei:
            w.ws.poll()
        assert ei.value.code == aclgpu.ERR_DEPTH
        w.rows_match()  # rows and baseline as they were
        w.write([(OP_DELETE, cycle[2]), (OP_TOUCH, ("pod", "p6", "banned", "user", "u0", ""))])
        got = w.poll_and_compare("cycle deleted")
        assert got == [(w0, 6, 0), (w1, w.e.find("pod", "p41"), 1)]
        w.rows_match()
    finally:
        w.close()


def test_two_logical_replicas(aclgpu):
    """An engine with two replicas of the snapshot on one device: a write followed by a poll sees the write, whichever replica the poll runs on."""
    w = World(aclgpu, SCHEMA_NS, devices=[0, 0])
    try:
        w.write([(OP_TOUCH, ("pod", f"a/p{i}", "namespace", "namespace", "a" if i % 2 else "b", "")) for i in range(50)])
        w0, w1 = w.add("u0"), w.add("u1")
        for step in range(8):
            op = OP_TOUCH if step < 4 else OP_DELETE
            w.write([(op, ("namespace", "ab"[step % 2], "viewer", "user", f"u{(step // 2) % 2}", ""))])
            assert len(w.poll_and_compare(step, py=False)) == 25
            w.e.check("pod", "a/p1", "view", "user", "u0")  # (other evaluations move the replicas' turn between the polls)
        assert len(w.e.replica_calls()) == 2
        w.rows_match()
    finally:
        w.close()


def test_watcher_subject_is_pinned(aclgpu, monkeypatch):
    """A watcher for a user without a single relationship, the recycling quarantine at zero for this engine (the knob is read when the schema is loaded):
    new names drain the free list, and the watched user's id is still its own -- a later grant is reported to that watcher."""
    monkeypatch.setenv("ACL_ID_QUARANTINE_MS", "0")
    w = World(aclgpu, SCHEMA_NS)
    monkeypatch.delenv("ACL_ID_QUARANTINE_MS")
    try:
        w.write([(OP_TOUCH, ("pod", f"a/p{i}", "namespace", "namespace", "a", "")) for i in range(5)])
        w0 = w.add("ghost")
        gid = w.e.find("user", "ghost")
        assert w.poll_and_compare("nothing yet", py=False) == []
        for i in range(10):  # subjects no relationship names: unpinned, theirs to lose at once
            assert w.e.lookup("pod", "view", "user", f"passer-by-{i}") == set()
        tmp = [("namespace", "b", "viewer", "user", f"tmp-{i}", "") for i in range(10)]
        w.write([(OP_TOUCH, r) for r in tmp])
        w.write([(OP_DELETE, r) for r in tmp])  # ten users lose their last relationship: ten free ids
        w.write([(OP_TOUCH, ("namespace", "b", "viewer", "user", f"new-{i}", "")) for i in range(30)])  # ... taken by new names, and more names than free ids
        assert w.e.stats()["ids_recycled"] >= 1 and w.e.find("user", "ghost") == gid
        w.write([(OP_TOUCH, ("namespace", "a", "viewer", "user", "ghost", ""))])
        assert w.poll_and_compare("granted", py=False) == [(w0, i, 1) for i in range(5)]
        w.rows_match()
    finally:
        w.close()

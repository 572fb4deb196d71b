"""Subject-direction watch sets on the GPU (csrc/engine_watchset.cpp subject_rows, kernels.hip k_refine_*): who gained or lost a permission on each
watched resource.  Every poll's records against the differences of rows that the ORACLES define -- for every subject name of the type, whether both the C
oracle's and the Python oracle's Check answer HAS -- never against the engine's own LookupSubjects.

A record is (watcher, subject id, gained, reserved); a poll's records are ordered by (watcher, subject id), so whole lists are compared.  The wildcard: a
resource whose permission a subject NOBODY NAMES holds (the oracles' Check of such a subject) is expected to carry the bit of the `*` object, reported by a
record with WATCH_CHANGE_WILDCARD; on a monotone permission the other bits of such a row are compared for the named subjects only."""
import numpy as np
import pytest

from oracle import orc
from oracle.pyoracle import PyOracle
from tests.watch_records import expected_records, records_of

pytestmark = pytest.mark.gpu

OP_TOUCH, OP_DELETE = 2, 3
WILD = "*"
NOBODY = "nobody-names-this-subject"


@pytest.fixture(scope="module")
def aclgpu(aclgpu_lib):
    import aclgpu as m
    return m


class Oracles:
    """The C oracle and the Python oracle under the same writes; holds() is their common answer."""

    def __init__(self, schema):
        self.o = orc.Oracle(schema)
        self.p = PyOracle(schema)

    def write(self, ups):
        for k in range(0, len(ups), 1000):
            self.o.write(ups[k:k + 1000])
        for u in ups:
            if u[0] == OP_DELETE:
                self.p.delete(*u[1])
            else:
                self.p.touch(*u[1], expires=u[2] if len(u) > 2 else 0)

    def set_now(self, t):
        self.o.set_now(t)
        self.p.now = t

    def holds(self, rt, rid, perm, st, sid):
        a = self.o.check(rt, rid, perm, st, sid) == (2, 0)
        b = self.p.check(rt, rid, perm, st, sid) == "HAS"
        return a and b


class World:
    """One engine and the oracles under the same writes; `held` is the row (a set of subject names, WILD among them) of every watcher at its last poll.
    `users`: every subject name of the type.  `named`: on a monotone permission, resource name -> the subjects named for it without the wildcard (the
    rows of such a permission keep those and the wildcard bit)."""

    def __init__(self, aclgpu, schema, users, rt="pod", perm="view", st="user", named=None, **kw):
        self.m = aclgpu
        self.e = aclgpu.Engine(schema, device=kw.pop("device", 0), **kw)
        self.x = Oracles(schema)
        self.rt, self.perm, self.st, self.users, self.named = rt, perm, st, list(users), named
        self.ws = self.e.subject_watch_set(rt, perm, st)
        self.resource, self.held = {}, {}

    def close(self):
        self.ws.close()
        self.e.close()

    def write(self, ups):
        for k in range(0, len(ups), 1000):
            self.e.write(ups[k:k + 1000])
        self.x.write(ups)

    def set_now(self, t):
        self.e.set_now(t)
        self.x.set_now(t)

    def row_of(self, rid):
        """the oracles' row of one resource"""
        wild = self.x.holds(self.rt, rid, self.perm, self.st, NOBODY)
        if wild and self.named is not None:
            row = set(self.named[rid])
            assert all(self.x.holds(self.rt, rid, self.perm, self.st, u) for u in row)
        else:
            row = {u for u in self.users if self.x.holds(self.rt, rid, self.perm, self.st, u)}
        return row | ({WILD} if wild else set())

    def add(self, rid, from_now=False):
        w = self.ws.add(rid, from_now=from_now)
        self.resource[w] = rid
        self.held[w] = None if from_now else set()
        return w

    def remove(self, w):
        self.ws.remove(w)
        del self.resource[w], self.held[w]

    def ids(self, names):
        out = sorted(self.e.find(self.st, n) for n in names)
        assert None not in out
        return out

    def expected(self):
        wid = self.e.find(self.st, WILD)
        after = {w: self.row_of(self.resource[w]) for w in sorted(self.resource)}
        recs = expected_records(self.held, after, lambda n: self.e.find(self.st, n), lambda i: self.m.WATCH_CHANGE_WILDCARD if i == wid else 0)
        return recs, after

    def poll_and_compare(self, tag=None):
        want, after = self.expected()
        rev, recs = self.ws.poll()
        got = records_of(recs, reserved=True)
        assert got == want, tag
        assert rev == self.e.revision
        self.held = after
        return got

    def rows_match(self):
        for w, rid in self.resource.items():
            assert self.ws.row(w).tolist() == self.ids(self.held[w]), (w, rid)


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
    """pod -> namespace -> group#member -> group#member -> user, 70 users (a row crosses a 32-bit word and a 64-bit pair), three watched pods, one of them
    FROM_NOW.  ONE group#member@user relationship: exactly the oracles' difference comes back -- and acl_watch_recheck for type pod hears nothing; the
    relationship deleted: the same records as lost; row() equals the oracles' row after every poll."""
    users = [f"u{i}" for i in range(70)]
    w = World(aclgpu, SCHEMA_NESTED, users)
    try:
        ups = []
        for n in range(3):
            ups += [(OP_TOUCH, ("namespace", f"ns{n}", "viewer", "group", f"top{n}", "member")), (OP_TOUCH, ("group", f"top{n}", "member", "group", f"mid{n}", "member")),
                    (OP_TOUCH, ("pod", f"ns{n}/p", "namespace", "namespace", f"ns{n}", ""))]
        ups += [(OP_TOUCH, ("group", f"mid{i % 3}", "member", "user", users[i], "")) for i in range(70)]
        w.write(ups)
        assert w.e.find("user", "u69") >= 64 and w.e.find("user", "u0") < 32
        w0, w1, w2 = w.add("ns0/p"), w.add("ns1/p"), w.add("ns2/p", from_now=True)
        base = w.poll_and_compare("baseline")
        assert len(base) == 24 + 23 and all(g == 1 and r == 0 for _w, _i, g, r in base) and {x[0] for x in base} == {w0, w1}
        assert min(x[1] for x in base) < 32 and max(x[1] for x in base) >= 64
        w.rows_match()
        assert len(w.held[w2]) == 23
        cursor = w.e.revision
        w.write([(OP_TOUCH, ("group", "mid1", "member", "user", "u69", ""))])  # u69 is in mid0: ns1/p gains it
        got = w.poll_and_compare("membership")
        assert got == [(w1, w.e.find("user", "u69"), 1, 0)]
        updates, _cur = w.e.watch_recheck(cursor, "pod", "view", "user", "u69")
        assert updates == []  # the reference-shaped watch path hears nothing: no update of type pod exists
        w.rows_match()
        w.write([(OP_DELETE, ("group", "mid1", "member", "user", "u69", ""))])
        assert w.poll_and_compare("membership deleted") == [(w1, w.e.find("user", "u69"), 0, 0)]
        w.rows_match()
        assert w.ws.stats() == {"polls": 3, "walks": 3, "changes": 49}
    finally:
        w.close()


SCHEMA_STREAM = """
definition user {}
definition group {
  relation member: user with expiration | group#member
}
definition pod {
  relation viewer: user | group#member
  relation banned: user
  permission view = viewer - banned
}
"""


def test_seeded_random_stream(aclgpu):
    """40 steps of touches, deletes and expiries over nested groups of 300 users, 8 watched pods, max_sub_batch=64 (the confirmation of a poll takes several
    slices): every poll equals the oracles' difference.  A watcher is added and one removed mid-stream; a poll with nothing changed walks nothing."""
    rng = np.random.default_rng(20261019)
    users, groups, pods = [f"u{i}" for i in range(300)], [f"g{i}" for i in range(12)], [f"p{i}" for i in range(9)]
    now = 1_800_000_000
    w = World(aclgpu, SCHEMA_STREAM, users, max_sub_batch=64)
    try:
        w.set_now(now)
        ups = [(OP_TOUCH, ("group", groups[i % 12], "member", "user", users[i], "")) for i in range(300)]
        ups += [(OP_TOUCH, ("group", groups[g], "member", "group", groups[g + 4], "member")) for g in range(8)]  # g0..3 <- g4..7 <- g8..11: no cycles
        ups += [(OP_TOUCH, ("pod", pods[k], "viewer", "group", groups[k % 4 if k < 6 else 4 + k % 4], "member")) for k in range(9)]
        w.write(ups)
        for k in range(7):
            w.add(pods[k], from_now=bool(k % 2))
        total = len(w.poll_and_compare("baseline"))
        live = []
        for step in range(40):
            if step == 12:
                w.add(pods[7])  # from the empty row
            if step == 22:
                w.remove(2)
            if step == 30:
                w.add(pods[8], from_now=True)
            kind = int(rng.integers(6))
            u, g, p = users[rng.integers(300)], groups[rng.integers(12)], pods[rng.integers(9)]
            if kind == 0 and live:
                ups = [(OP_DELETE, live.pop(int(rng.integers(len(live)))))]
            elif kind == 1:
                ups = [(OP_TOUCH, ("group", g, "member", "user", u, ""), now + 10 * (step + 1) + 5)]  # runs out two or three steps on
            else:
                rel = [("pod", p, "banned", "user", u, ""), ("pod", p, "viewer", "user", u, ""), ("group", g, "member", "user", u, ""),
                       ("pod", p, "viewer", "group", g, "member")][kind % 4]
                ups = [(OP_TOUCH, rel)]
                if rel not in live:
                    live.append(rel)
            w.write(ups)
            if step % 3 == 2:
                w.set_now(now + 10 * (step + 1))
            total += len(w.poll_and_compare((step, ups)))
            if step == 20:  # nothing changed since: no walk
                before = w.ws.stats()
                rev, recs = w.ws.poll()
                after = w.ws.stats()
                assert recs.size == 0 and rev == w.e.revision and after["walks"] == before["walks"] and after["polls"] == before["polls"] + 1
        assert total > 300 and len(w.resource) == 8
        w.rows_match()
    finally:
        w.close()


SCHEMA_FLAT = """
definition user {}
definition pod {
  relation viewer: user
  permission view = viewer
}
"""


def test_width_growth(aclgpu):
    """120 subjects at the baseline (one 16-byte row unit), 140 at the next poll (two): the old rows are read with the narrower stride and the new ids
    appear as gains only where granted."""
    users = [f"u{i}" for i in range(140)]
    w = World(aclgpu, SCHEMA_FLAT, users[:120])
    try:
        w.write([(OP_TOUCH, ("pod", f"p{i % 3}", "viewer", "user", users[i], "")) for i in range(120)])
        assert w.e.object_count("user") == 120
        w0, w1, w2 = w.add("p0"), w.add("p1"), w.add("p2", from_now=True)
        assert len(w.poll_and_compare("baseline")) == 80
        w.rows_match()
        w.users = users
        w.write([(OP_TOUCH, ("pod", "p1" if i % 2 else "p2", "viewer", "user", users[i], "")) for i in range(120, 140)] + [(OP_DELETE, ("pod", "p1", "viewer", "user", "u1", ""))])
        assert w.e.object_count("user") == 140
        got = w.poll_and_compare("grown")
        assert [x for x in got if x[0] == w1] == [(w1, 1, 0, 0)] + [(w1, i, 1, 0) for i in range(121, 140, 2)]
        assert [x for x in got if x[0] == w2] == [(w2, i, 1, 0) for i in range(120, 140, 2)] and not [x for x in got if x[0] == w0]
        w.rows_match()
        assert w.poll_and_compare("again") == []
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


def ban_world(aclgpu, **kw):
    """four pods of 40 viewers each (through a group for two of them), max_sub_batch=64: a poll's confirmation takes several slices"""
    users = [f"u{i}" for i in range(60)]
    w = World(aclgpu, SCHEMA_BAN, users, max_sub_batch=64, **kw)
    ups = [(OP_TOUCH, ("group", "team", "member", "user", users[i], "")) for i in range(40)]
    ups += [(OP_TOUCH, ("pod", "p0", "viewer", "group", "team", "member")), (OP_TOUCH, ("pod", "p1", "viewer", "group", "team", "member"))]
    ups += [(OP_TOUCH, ("pod", p, "viewer", "user", users[i], "")) for p in ("p2", "p3") for i in range(20, 60)]
    w.write(ups)
    return w


def test_exclusion_is_confirmed_on_the_device(aclgpu):
    """view = viewer - banned: a ban reports a loss, an unban a gain, for the banned pod alone."""
    w = ban_world(aclgpu)
    try:
        ws = [w.add(f"p{k}") for k in range(4)]
        assert len(w.poll_and_compare("baseline")) == 160
        w.write([(OP_TOUCH, ("pod", "p0", "banned", "user", "u3", "")), (OP_TOUCH, ("pod", "p2", "banned", "user", "u33", "")), (OP_TOUCH, ("pod", "p2", "banned", "user", "u59", ""))])
        assert w.poll_and_compare("banned") == [(ws[0], w.e.find("user", "u3"), 0, 0), (ws[2], w.e.find("user", "u33"), 0, 0), (ws[2], w.e.find("user", "u59"), 0, 0)]
        w.rows_match()
        w.write([(OP_DELETE, ("pod", "p2", "banned", "user", "u33", ""))])
        assert w.poll_and_compare("unbanned") == [(ws[2], w.e.find("user", "u33"), 1, 0)]
        w.rows_match()
    finally:
        w.close()


CYCLE = [("pod", "p1", "banned", "group", "ga", "member"), ("group", "ga", "member", "group", "gb", "member"), ("group", "gb", "member", "group", "ga", "member")]


def test_a_failed_confirmation_keeps_the_baseline(aclgpu):
    """A cycle of groups behind p1's `banned`: its candidates' confirming Check runs into the depth limit, the poll fails with ERR_DEPTH and row() still shows
    the baseline; the cycle deleted: the next poll reports the whole difference, a change written while the poll was failing included."""
    w = ban_world(aclgpu)
    try:
        ws = [w.add(f"p{k}") for k in range(4)]
        assert len(w.poll_and_compare("baseline")) == 160
        w.write([(OP_TOUCH, r) for r in CYCLE] + [(OP_TOUCH, ("pod", "p3", "banned", "user", "u40", ""))])
        assert w.x.p.check("pod", "p1", "view", "user", "u0") == "ERR"
        with pytest.raises(aclgpu.AclError) as ei:
            w.ws.poll()
        assert ei.value.code == aclgpu.ERR_DEPTH and "resource id" in str(ei.value)
        w.rows_match()  # rows and baseline as they were
        w.write([(OP_DELETE, CYCLE[2]), (OP_TOUCH, ("pod", "p0", "banned", "user", "u7", ""))])
        assert w.poll_and_compare("cycle deleted") == [(ws[0], w.e.find("user", "u7"), 0, 0), (ws[3], w.e.find("user", "u40"), 0, 0)]
        w.rows_match()
    finally:
        w.close()


def test_lenient_lookup_leaves_an_erring_candidate_out(aclgpu):
    w = ban_world(aclgpu, lenient_lookup=True)
    try:
        ws = [w.add(f"p{k}") for k in range(4)]
        assert len(w.poll_and_compare("baseline")) == 160
        w.write([(OP_TOUCH, r) for r in CYCLE])
        got = w.poll_and_compare("cycle")  # every candidate of p1 errs: none of them holds it by the oracles either
        assert len(got) == 40 and all(x[0] == ws[1] and x[2] == 0 for x in got)
        w.rows_match()
    finally:
        w.close()


SCHEMA_AND = """
definition user {}
definition namespace {
  relation viewer: user
  permission view = viewer
}
definition pod {
  relation namespace: namespace
  relation creator: user
  permission strict = creator & namespace->view
}
"""

SCHEMA_ALL = """
definition user {}
definition folder {
  relation viewer: user
  relation banned: user
  permission view = viewer - banned
}
definition doc {
  relation parent: folder
  permission view_all = parent.all(view)
}
"""


def test_intersection_is_confirmed_on_the_device(aclgpu):
    """strict = creator & namespace->view (the positive relaxation walks creator + namespace->view): one poll after a write that flips a few subjects."""
    users = [f"u{i}" for i in range(45)]
    w = World(aclgpu, SCHEMA_AND, users, perm="strict", max_sub_batch=64)
    try:
        ups = [(OP_TOUCH, ("pod", f"p{k}", "namespace", "namespace", "ns", "")) for k in range(3)]
        ups += [(OP_TOUCH, ("pod", f"p{k}", "creator", "user", users[i], "")) for k in range(3) for i in range(k, 45, 2)]
        ups += [(OP_TOUCH, ("namespace", "ns", "viewer", "user", users[i], "")) for i in range(0, 45, 3)]
        w.write(ups)
        for k in range(3):
            w.add(f"p{k}")
        assert len(w.poll_and_compare("baseline")) > 15
        w.rows_match()
        w.write([(OP_TOUCH, ("namespace", "ns", "viewer", "user", "u1", "")), (OP_TOUCH, ("namespace", "ns", "viewer", "user", "u4", "")),
                 (OP_DELETE, ("namespace", "ns", "viewer", "user", "u6", ""))])
        assert len(w.poll_and_compare("flip")) >= 3
        w.rows_match()
    finally:
        w.close()


def test_all_arrow_is_confirmed_on_the_device(aclgpu):
    """view_all = parent.all(view) over folders with bans: one poll after a write that flips a few subjects."""
    users = [f"u{i}" for i in range(45)]
    w = World(aclgpu, SCHEMA_ALL, users, rt="doc", perm="view_all", max_sub_batch=64)
    try:
        ups = [(OP_TOUCH, ("doc", f"d{k}", "parent", "folder", f"f{j}", "")) for k in range(3) for j in (k, k + 1)]
        ups += [(OP_TOUCH, ("folder", f"f{j}", "viewer", "user", users[i], "")) for j in range(4) for i in range(45) if (i + j) % 5]
        ups += [(OP_TOUCH, ("folder", "f1", "banned", "user", "u2", ""))]
        w.write(ups)
        for k in range(3):
            w.add(f"d{k}")
        assert len(w.poll_and_compare("baseline")) > 40
        w.rows_match()
        w.write([(OP_TOUCH, ("folder", "f2", "banned", "user", "u11", "")), (OP_DELETE, ("folder", "f1", "banned", "user", "u2", "")),
                 (OP_TOUCH, ("folder", "f0", "viewer", "user", "u0", ""))])
        assert len(w.poll_and_compare("flip")) >= 4
        w.rows_match()
    finally:
        w.close()


SCHEMA_WILD = """
definition user {}
definition pod {
  relation viewer: user | user:*
  permission view = viewer
}
"""

SCHEMA_WILD_BAN = """
definition user {}
definition pod {
  relation viewer: user | user:*
  relation banned: user
  permission view = viewer - banned
}
"""


def test_wildcard_on_a_monotone_permission(aclgpu):
    """viewer: user | user:* -- granting and deleting user:* gives exactly ONE flagged record per watcher; the named viewers are unaffected."""
    users = [f"u{i}" for i in range(40)]
    named = {"p0": {users[i] for i in range(0, 40, 2)}, "p1": {"u1", "u39"}, "p2": set()}
    w = World(aclgpu, SCHEMA_WILD, users, named=named)
    try:
        w.write([(OP_TOUCH, ("pod", p, "viewer", "user", u, "")) for p in named for u in sorted(named[p])])
        ws = [w.add(p) for p in ("p0", "p1", "p2")]
        assert len(w.poll_and_compare("baseline")) == 22
        wid = w.e.find("user", WILD)
        w.write([(OP_TOUCH, ("pod", p, "viewer", "user", "*", "")) for p in ("p0", "p1", "p2")])
        assert w.poll_and_compare("granted") == [(x, wid, 1, aclgpu.WATCH_CHANGE_WILDCARD) for x in ws]
        w.rows_match()
        w.write([(OP_DELETE, ("pod", p, "viewer", "user", "*", "")) for p in ("p0", "p2")])
        assert w.poll_and_compare("deleted") == [(ws[0], wid, 0, aclgpu.WATCH_CHANGE_WILDCARD), (ws[2], wid, 0, aclgpu.WATCH_CHANGE_WILDCARD)]
        w.rows_match()
    finally:
        w.close()


def test_wildcard_under_an_exclusion(aclgpu):
    """view = viewer - banned with user:* -- every unbanned existing user is in the row; a ban gives one loss, an unban one gain; user:* deleted: everyone
    but the named viewers is lost."""
    users = [f"u{i}" for i in range(70)]
    w = World(aclgpu, SCHEMA_WILD_BAN, users, max_sub_batch=64)
    try:
        w.write([(OP_TOUCH, ("pod", "p9", "viewer", "user", u, "")) for u in users] + [(OP_TOUCH, ("pod", "p1", "viewer", "user", u, "")) for u in users[:3]]
                + [(OP_TOUCH, ("pod", "p0", "viewer", "user", "*", "")), (OP_TOUCH, ("pod", "p0", "viewer", "user", "u2", "")), (OP_TOUCH, ("pod", "p0", "banned", "user", "u9", ""))])
        w0, w1 = w.add("p0"), w.add("p1")
        wid = w.e.find("user", WILD)
        base = w.poll_and_compare("baseline")
        assert len(base) == 70 + 3 and (w0, wid, 1, aclgpu.WATCH_CHANGE_WILDCARD) in base and (w0, w.e.find("user", "u9"), 1, 0) not in base
        w.rows_match()
        w.write([(OP_TOUCH, ("pod", "p0", "banned", "user", "u66", ""))])
        assert w.poll_and_compare("ban") == [(w0, w.e.find("user", "u66"), 0, 0)]
        w.write([(OP_DELETE, ("pod", "p0", "banned", "user", "u9", ""))])
        assert w.poll_and_compare("unban") == [(w0, w.e.find("user", "u9"), 1, 0)]
        w.rows_match()
        w.write([(OP_DELETE, ("pod", "p0", "viewer", "user", "*", ""))])
        got = w.poll_and_compare("wildcard deleted")
        assert len(got) == 69 and all(x[0] == w0 and x[2] == 0 for x in got) and w.held[w0] == {"u2"}
        w.rows_match()
    finally:
        w.close()


_WIDE = {}


def wide_graph():
    """a random ban-schema graph of 2 000 users and 64 pods, and the oracles' rows of the pods (computed once for both engine configurations)"""
    if not _WIDE:
        rng = np.random.default_rng(7)
        users, pods = [f"u{i}" for i in range(2000)], [f"p{k}" for k in range(64)]
        ups = [(OP_TOUCH, ("group", f"g{i % 20}", "member", "user", users[i], "")) for i in range(0, 2000, 3)]
        ups += [(OP_TOUCH, ("group", f"g{g}", "member", "group", f"g{g + 10}", "member")) for g in range(10)]
        ups += [(OP_TOUCH, ("pod", "unwatched", "viewer", "user", u, "")) for u in users]  # (every user exists: a relationship names it)
        for k, p in enumerate(pods):
            ups += [(OP_TOUCH, ("pod", p, "viewer", "group", f"g{int(g)}", "member")) for g in rng.choice(20, size=1 + k % 2, replace=False)]
            ups += [(OP_TOUCH, ("pod", p, "viewer", "user", users[int(i)], "")) for i in rng.choice(2000, size=12, replace=False)]
            ups += [(OP_TOUCH, ("pod", p, "banned", "user", users[int(i)], "")) for i in rng.choice(2000, size=150, replace=False)]
            if k % 16 == 5:
                ups.append((OP_TOUCH, ("pod", p, "banned", "group", f"g{k % 20}", "member")))
        x = Oracles(SCHEMA_BAN)
        x.write(ups)
        want = np.zeros((64, 2000), dtype=bool)
        for k, p in enumerate(pods):
            for i, u in enumerate(users):
                want[k, i] = x.holds("pod", p, "view", "user", u)
        _WIDE.update(users=users, pods=pods, ups=ups, want=want, x=x)
    return _WIDE


@pytest.mark.parametrize("max_sub_batch", [64, None])
def test_device_path_against_the_oracles_at_width(aclgpu, max_sub_batch):
    """acl_selfcheck_subject_rows for 64 pods of a random ban-schema graph of 2 000 users: every row equals the oracles' per-subject Check, with the
    confirmation cut into slices of 64 and in one piece."""
    g = wide_graph()
    kw = {} if max_sub_batch is None else {"max_sub_batch": max_sub_batch}
    with aclgpu.Engine(SCHEMA_BAN, device=0, **kw) as e:
        for k in range(0, len(g["ups"]), 1000):
            e.write(g["ups"][k:k + 1000])
        rids = np.array([e.find("pod", p) for p in g["pods"]], dtype=np.uint32)
        rows = e.selfcheck_subject_rows("pod", "view", "user", "", rids)
        bits = np.unpackbits(rows.view(np.uint8), axis=1, bitorder="little").astype(bool)
        uid = np.array([e.find("user", u) for u in g["users"]])
        assert e.object_count("user") == 2000 and not bits[:, 2000:].any()
        got = bits[:, uid]
        assert np.array_equal(got, g["want"]) and 100 < g["want"].sum() < 64 * 1000


def test_two_logical_replicas(aclgpu):
    """An engine with two replicas of the snapshot on one device: a write followed by a poll sees the write, whichever replica the poll runs on."""
    users = [f"u{i}" for i in range(10)]
    w = World(aclgpu, SCHEMA_FLAT, users, devices=[0, 0])
    try:
        w0, w1 = w.add("p0"), w.add("p1")
        for step in range(8):
            op = OP_TOUCH if step < 4 else OP_DELETE
            w.write([(op, ("pod", f"p{step % 2}", "viewer", "user", users[(step // 2) % 2], ""))])
            assert len(w.poll_and_compare(step)) == 1
            w.e.check("pod", "p0", "view", "user", "u0")  # (other evaluations move the replicas' turn between the polls)
        assert len(w.e.replica_calls()) == 2
        w.rows_match()
    finally:
        w.close()


def test_refusals_and_the_poll_loop(aclgpu, aclgpu_lib):
    """The resource-direction add contract is unchanged beside a subject-direction set; one run_watch_set loop per set; closing an unknown set is refused;
    a deadline of 1 ns fails the poll and keeps the baseline."""
    import ctypes as C
    from aclgpu import client
    L = aclgpu_lib
    users = [f"u{i}" for i in range(5)]
    w = World(aclgpu, SCHEMA_FLAT, users)
    try:
        w.write([(OP_TOUCH, ("pod", "p0", "viewer", "user", "u0", "")), (OP_TOUCH, ("pod", "p1", "viewer", "user", "u1", ""))])
        # a resource-direction set of the same engine: add takes a SUBJECT, its records carry resource ids and no flag
        rs = w.e.watch_set("pod", "view", "user")
        r0 = rs.add("u0")
        _rev, recs = rs.poll()
        assert [(int(r["watcher"]), int(r["resource_id"]), int(r["gained"]), int(r["reserved"])) for r in recs] == [(r0, w.e.find("pod", "p0"), 1, 0)]
        x = C.c_uint32()
        assert L.acl_watch_set_add(w.e._h, rs._s, b"not an id", 0, C.byref(x)) == aclgpu.ERR_INVALID_ARGUMENT
        assert L.acl_watch_set_add(w.e._h, w.ws._s, b"not an id", 0, C.byref(x)) == aclgpu.ERR_INVALID_ARGUMENT  # ... and the same validation of a resource id
        assert L.acl_watch_set_add(w.e._h, w.ws._s, b"p0", 2, C.byref(x)) == aclgpu.ERR_INVALID_ARGUMENT
        rs.close()
        w0 = w.add("p0")
        # the one poll loop of the set: names resolved in the SUBJECT type
        got = []
        loop = client.run_watch_set(w.e, w.ws, {w0: lambda allowed, name: got.append((allowed, name))}, polls=1)
        first = next(loop)
        with pytest.raises(aclgpu.AclError) as ei:
            next(client.run_watch_set(w.e, w.ws, {}, polls=1))
        assert ei.value.code == aclgpu.ERR_FAILED_PRECONDITION
        assert [first] + list(loop) == [(True, "u0", w0)] and got == [(True, "u0")]
        w.held[w0] = {"u0"}
        # closing a set the engine does not know
        assert L.acl_watch_set_close(w.e._h, C.c_void_p(0x1000)) == aclgpu.ERR_INVALID_ARGUMENT
        # a deadline that has passed before the poll starts: the poll fails, the baseline stays
        w.write([(OP_TOUCH, ("pod", "p0", "viewer", "user", "u3", ""))])
        with pytest.raises(aclgpu.AclError) as ei:
            w.ws.poll(timeout_s=1e-9)
        assert ei.value.code == aclgpu.ERR_DEADLINE_EXCEEDED
        w.rows_match()
        assert w.poll_and_compare("after the deadline") == [(w0, w.e.find("user", "u3"), 1, 0)]
    finally:
        w.close()


def test_a_ban_that_runs_out_grants_with_no_write(aclgpu):
    """`view = (viewer + creator + namespace->view) - banned` with `banned: user with expiration` (tools/fuzz_gpu.py SCHEMA_COMBINE_EXPIRING): a ban's expiry
    GRANTS.  One pod watched in the subject direction; the bans of a direct viewer and of a viewer through the namespace run out with no write -- the poll (the
    device path's confirmation, k_refine_*) reports both as gained, against both oracles; a ban without an expiry stays.  The clock set back: both lost again."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("fuzz_gpu", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "fuzz_gpu.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    users = [f"u{i}" for i in range(20)]
    t0 = 1_700_000_000
    w = World(aclgpu, fz.SCHEMA_COMBINE_EXPIRING, users)
    try:
        w.set_now(t0)
        ups = [(OP_TOUCH, ("pod", "p0", "namespace", "namespace", "n0", ""))]
        ups += [(OP_TOUCH, ("pod", "p0", "viewer", "user", f"u{i}", "")) for i in range(10)]
        ups += [(OP_TOUCH, ("namespace", "n0", "viewer", "user", f"u{i}", "")) for i in range(10, 15)]
        ups += [(OP_TOUCH, ("pod", "p0", "banned", "user", "u3", ""), t0 + 100), (OP_TOUCH, ("pod", "p0", "banned", "user", "u12", ""), t0 + 100),
                (OP_TOUCH, ("pod", "p0", "banned", "user", "u5", "")), (OP_TOUCH, ("pod", "p0", "banned", "user", "u17", ""), t0 + 100)]
        w.write(ups)
        ws = w.add("p0")
        assert len(w.poll_and_compare("baseline")) == 12  # (15 viewers, three of them banned)
        w.rows_match()
        rev = w.e.revision
        w.set_now(t0 + 150)
        assert w.poll_and_compare("the bans ran out") == [(ws, i, 1, 0) for i in sorted((w.e.find("user", "u3"), w.e.find("user", "u12")))]
        w.rows_match()
        w.set_now(t0 + 50)
        assert w.poll_and_compare("the clock set back") == [(ws, i, 0, 0) for i in sorted((w.e.find("user", "u3"), w.e.find("user", "u12")))]
        w.rows_match()
        assert w.e.revision == rev  # (no write in between)
    finally:
        w.close()

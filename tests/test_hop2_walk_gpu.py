"""The single-launch walk on two-hop rows (kernels.hip process_segment's direct form; plan.hpp Snapshot::hop2_*), equal to the oracle item by item, answers and
error codes, with the rows in use and -- in a fresh engine under ACL_HOP2=0 -- on the one-hop rows alone.

Graphs are built from explicit nesting lists over SCHEMA_C4; group ids are handed out parent by parent, so a row's order is the order of construction.
  family(m, a, b)  pod p0 viewed by m top groups T; every T has a children X, every X b children Y, every Y one child Z, every Z one leaf W: the T rows are
                   two-hop (a + a b <= 16 ids), the Y's they push are expanded two-hop again (Z, then W).  m covers one segment, one pair, several pairs and the
                   boundaries of 64 and 128 entries; (4, 3) is a full row of 16, and 128 of them fill the 2 048-child window of a pair exactly.
  Subjects are members of exactly one group: at T, X (the first work item), Y (the last valid lane of the last window; the first grandchild of a row), Z, W --
  and one of nothing.  Every subject is asked alone (1-item batches), all together in a 4 096-item batch, and for (m, a, b) = (129, 1, 1) and (2, 4, 3) in a 65 536-item batch (12-wave blocks).
Then: rows of 17 ids (one-hop) interleaved with two-hop ones; a pair whose two-hop rows overflow the window while its one-hop rows fit (answered inside the walk,
no retry); the same groups reached from the pod and through its namespace (two levels in one iteration); chains and cycles at the depth limit; writes between
two batches (a nesting write drops the rows with a patch, a membership write keeps them)."""
import numpy as np
import pytest

from aclgpu.workloads import SCHEMA_C4
from oracle import orc

pytestmark = pytest.mark.gpu

N_USER = 24


@pytest.fixture(scope="module")
def aclgpu(aclgpu_lib):
    import aclgpu as m
    return m


def u32(a):
    return np.asarray(a, dtype=np.uint32)


class Graph:
    def __init__(self):
        self.ng = 0
        self.nest, self.mem = [], []          # (parent group, child group), (group, user)
        self.pod_view, self.ns_view = [], []  # (pod, group), (namespace, group)
        self.pod_ns = []                      # (pod, namespace)
        self.npod, self.nns = 1, 0

    def new(self, n):
        ids = list(range(self.ng, self.ng + n))
        self.ng += n
        return ids

    def kids(self, parents, k):
        """k new children under every parent, ids ascending parent by parent"""
        out = []
        for p in parents:
            c = self.new(k)
            self.nest += [(p, x) for x in c]
            out += c
        return out

    def place(self, groups):
        """user i becomes a member of groups[i]; the users behind them are members of nothing"""
        assert len(groups) < N_USER
        self.mem += [(g, i) for i, g in enumerate(groups)]

    def load(self, t):
        for k in range(N_USER):
            assert t.intern("user", f"u{k}") == k
        for i in range(self.ng + 8):  # (a few spare groups for the write tests)
            assert t.intern("group", f"g{i}") == i
        for i in range(self.npod):
            assert t.intern("pod", f"p{i}") == i
        for i in range(self.nns):
            assert t.intern("namespace", f"n{i}") == i
        for rt, rel, st, sr, pairs in (("group", "member", "group", "member", self.nest), ("group", "member", "user", "", self.mem),
                                       ("pod", "viewer", "group", "member", self.pod_view), ("namespace", "viewer", "group", "member", self.ns_view),
                                       ("pod", "namespace", "namespace", "", self.pod_ns)):
            if pairs:
                t.add_edges(rt, rel, st, sr, u32([a for a, _ in pairs]), u32([b for _, b in pairs]))


def family(m, a, b):
    g = Graph()
    T = g.new(m)
    g.pod_view = [(0, t) for t in T]
    X = g.kids(T, a)
    Y = g.kids(X, b)
    Z = g.kids(Y, 1)
    W = g.kids(Z, 1)
    g.place([T[-1], X[0], Y[-1], Y[(m // 2) * a * b], Z[0], W[-1], Z[-1], W[0], T[0], X[-1], Y[0], W[len(W) // 2]])
    return g


def expected(g, pods=(0,)):
    """-> (res, subj, perm, err) of every (pod, user) pair, from the oracle, computed once per graph"""
    o = orc.Oracle(SCHEMA_C4)
    g.load(o)
    res = np.repeat(u32(pods), N_USER)
    subj = np.tile(np.arange(N_USER, dtype=np.uint32), len(pods))
    perm, err = o.check_bulk_ids("pod", "view", res, "user", "", subj)
    return o, res, subj, perm, err


def run(aclgpu, monkeypatch, g, exp, sizes=(1, 4096), hop2=True, want_rows=True, between=None):
    """one fresh engine: every pair alone (size 1) and tiled into batches of the other sizes; -> stats"""
    _o, res, subj, perm, err = exp
    if hop2:
        monkeypatch.delenv("ACL_HOP2", raising=False)
    else:
        monkeypatch.setenv("ACL_HOP2", "0")
    with aclgpu.Engine(SCHEMA_C4, device=0) as e:
        g.load(e)
        e.stats_reset()
        for size in sizes:
            if size == 1:
                for i in range(res.size):
                    p, er = e.check_bulk_ids(e.make_items("pod", "view", res[i:i + 1], "user", "", subj[i:i + 1]))
                    assert p[0] == perm[i] and er[0] == err[i], (hop2, i, int(res[i]), int(subj[i]), p, perm[i], er, err[i])
            else:
                k = np.arange(size) % res.size
                p, er = e.check_bulk_ids(e.make_items("pod", "view", res[k], "user", "", subj[k]))
                assert np.array_equal(p, perm[k]) and np.array_equal(er, err[k]), (hop2, size, int((p != perm[k]).sum()), int((er != err[k]).sum()), np.flatnonzero(p != perm[k])[:8])
        st = e.stats()
        assert st["local_passes"] > 0 and st["expand_launches"] == 0 and st["overflow_retries"] == 0, st
        assert (st["hop2_rows"] > 0) == want_rows, st
        if between:
            between(e, st)
    return st


def both(aclgpu, monkeypatch, g, pods=(0,), sizes=(1, 4096)):
    exp = expected(g, pods)
    assert (exp[3] == orc.PERM_HAS).any() and (exp[3] != orc.PERM_HAS).any()
    run(aclgpu, monkeypatch, g, exp, sizes, hop2=True)
    run(aclgpu, monkeypatch, g, exp, sizes, hop2=False)
    return exp


@pytest.mark.parametrize("a,b", [(1, 1), (2, 3), (4, 3)])
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 127, 128, 129, 193])
def test_family(aclgpu, monkeypatch, m, a, b):
    g = family(m, a, b)
    # (the wide batch where a request's frontier stays small: 65 536 requests with 129 full rows each would outgrow the blocks' private regions on either row set)
    exp = both(aclgpu, monkeypatch, g, sizes=(1, 4096, 65536) if (m, a, b) in ((129, 1, 1), (2, 4, 3)) else (1, 4096))
    want = np.zeros(N_USER, dtype=bool)
    want[:12] = True
    assert np.array_equal(exp[3] == orc.PERM_HAS, want) and not exp[4].any()


def test_one_hop_rows_of_17_between_two_hop_rows(aclgpu, monkeypatch):
    g = Graph()
    T = g.new(130)
    g.pod_view = [(0, t) for t in T]
    hit = []
    for i, t in enumerate(T):
        X = g.kids([t], 4)
        Y = g.kids(X[:3], 3) + g.kids(X[3:], 3 if i % 2 == 0 else 4)  # 4 + 12 = 16: two-hop; 4 + 13 = 17: one-hop
        W = g.kids(Y, 1)
        if i in (0, 1, 64, 127, 128, 129):
            hit += [Y[-1], W[-1]]
    g.place(hit + [T[5]])
    both(aclgpu, monkeypatch, g)


def test_window_fallback_inside_the_walk(aclgpu, monkeypatch):
    """100 T's with two-hop rows of 16 (one-hop length 4) and 28 T's with one-hop rows of 20 leaves in ONE pair of segments: 2 160 children on the two-hop
    descriptors, beyond the 2 048 of the head-bit window, 960 on the one-hop ones -- the pair is expanded again from those, without a retry"""
    g = Graph()
    T = g.new(128)
    g.pod_view = [(0, t) for t in T]
    hit = []
    for i, t in enumerate(T):
        if i % 32 < 25:  # 4 x 25 = 100
            X = g.kids([t], 4)
            Y = g.kids(X, 3)
            W = g.kids(Y, 1)
            if i in (0, 120):
                hit += [X[0], Y[-1], W[-1]]
        else:            # 4 x 7 = 28
            L = g.kids([t], 20)
            if i in (25, 127):
                hit += [L[0], L[-1]]
    assert sum(1 for i in range(128) if i % 32 < 25) == 100
    g.place(hit)
    both(aclgpu, monkeypatch, g)


def test_two_levels_in_one_iteration(aclgpu, monkeypatch):
    """the pod's own viewers and its namespace's: the namespace's groups enter the frontier one level later than the pod's, so the iterations behind hold
    group#member states of two adjacent levels side by side, interleaved"""
    g = Graph()
    g.nns = 1
    g.pod_ns = [(0, 0)]
    T = g.new(70)
    X = g.kids(T, 2)
    Y = g.kids(X, 3)
    Z = g.kids(Y, 1)
    W = g.kids(Z, 2)
    V = g.kids(W[:40], 1)
    g.pod_view = [(0, t) for t in T[:50]] + [(0, y) for y in Y[:30]]
    g.ns_view = [(0, t) for t in T[20:]] + [(0, x) for x in X[:25]] + [(0, Z[-1])]
    g.place([T[0], T[-1], X[-1], Y[-1], Y[200], Z[-1], Z[100], W[-1], W[0], V[-1], V[0], X[60], W[333]])
    both(aclgpu, monkeypatch, g)


def _depth_graph(nest, ngroups, users_at):
    g = Graph()
    g.new(ngroups)
    g.nest = list(nest)
    g.npod, g.nns = 2, 1
    g.pod_view = [(0, 0)]   # pod p0: the chain starts at level 1 ...
    g.pod_ns = [(1, 0)]     # ... pod p1 reaches it through its namespace, one level further on: the other parity
    g.ns_view = [(0, 0)]
    g.place(users_at)
    return g


@pytest.mark.parametrize("shape", ["chain", "cycle2", "cycle3"])
def test_depth_limit(aclgpu, monkeypatch, shape):
    if shape == "chain":
        g = _depth_graph([(i, i + 1) for i in range(55)], 56, list(range(44, 56)))
    elif shape == "cycle2":
        g = _depth_graph([(0, 1), (1, 0)], 3, [1, 0])
    else:
        g = _depth_graph([(0, 1), (1, 2), (2, 0)], 4, [2])
    exp = expected(g, pods=(0, 1))
    perm, err = exp[3], exp[4]
    assert (perm == orc.PERM_HAS).any() and (err == orc.ERR_DEPTH).any()  # (some subject is out of reach of the 50 dispatches)
    if shape == "chain":
        assert (perm[:12] == orc.PERM_HAS).any() and (err[:12] == orc.ERR_DEPTH).any() and not np.array_equal(err[:N_USER], err[N_USER:])
    run(aclgpu, monkeypatch, g, exp, (1, 4096), hop2=True)
    run(aclgpu, monkeypatch, g, exp, (1, 4096), hop2=False)


def test_writes_between_two_batches(aclgpu, monkeypatch):
    g = family(65, 2, 3)
    exp = expected(g)
    o = exp[0]
    spare = g.ng  # g<spare>: interned, no relationships yet
    free = int(np.flatnonzero(exp[3] != orc.PERM_HAS)[0])

    def between(e, st0):
        # a user-membership write: a patch that keeps the rows
        up = [("group", f"g{g.ng - 1}", "member", "user", f"u{free}", "")]
        e.write([(aclgpu.OP_TOUCH, r) for r in up])
        o.write([(orc.OP_TOUCH, r) for r in up])
        res, subj = exp[1], exp[2]
        k = np.arange(4096) % res.size
        op, oe = o.check_bulk_ids("pod", "view", res, "user", "", subj)
        assert op[free] == orc.PERM_HAS
        p, er = e.check_bulk_ids(e.make_items("pod", "view", res[k], "user", "", subj[k]))
        assert np.array_equal(p, op[k]) and np.array_equal(er, oe[k])
        st1 = e.stats()
        assert st1["snapshot_patches"] > st0["snapshot_patches"] and st1["snapshot_builds"] == st0["snapshot_builds"] and st1["hop2_rows"] == st0["hop2_rows"] > 0, (st0, st1)
        # a nesting write: the last W gains a child that holds another user -- answers follow, the rows are dropped with the patch
        up = [("group", f"g{g.ng - 1}", "member", "group", f"g{spare}", "member"), ("group", f"g{spare}", "member", "user", f"u{free + 1}", "")]
        e.write([(aclgpu.OP_TOUCH, r) for r in up])
        o.write([(orc.OP_TOUCH, r) for r in up])
        op, oe = o.check_bulk_ids("pod", "view", res, "user", "", subj)
        assert op[free + 1] == orc.PERM_HAS
        p, er = e.check_bulk_ids(e.make_items("pod", "view", res[k], "user", "", subj[k]))
        assert np.array_equal(p, op[k]) and np.array_equal(er, oe[k]), (int((p != op[k]).sum()), np.flatnonzero(p != op[k])[:8])
        st2 = e.stats()
        assert st2["snapshot_patches"] > st1["snapshot_patches"] and st2["snapshot_builds"] == st1["snapshot_builds"] and st2["hop2_rows"] == 0, (st1, st2)
        assert st2["expand_launches"] == 0 and st2["overflow_retries"] == 0, st2

    run(aclgpu, monkeypatch, g, exp, (4096,), hop2=True, between=between)


def _fuzz_tool():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("fuzz_gpu", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "fuzz_gpu.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    return fz


def expiring_family():
    """family(2, 4, 3) for SCHEMA_C4_EXPIRING with two nestings that run out: T[0] -> X[0] at +100 s (under two-hop row T[0]: the users at X[0], Y[0], Z[0] and
    W[0] hang below it) and Y[-1] -> Z[-1] at +200 s (the grandchild hop of the row X[-1] pushes; the users at Z[-1] and W[-1] below it, the one AT Y[-1] stays).
    -> (graph, [(relationship text, seconds after the start)], {seconds after the start: the users 0..11 that have lost the pod then})"""
    g = family(2, 4, 3)
    T, X, Y, Z = [0, 1], list(range(2, 10)), list(range(10, 34)), list(range(34, 58))
    assert (T[0], X[0]) in g.nest and (Y[-1], Z[-1]) in g.nest
    ups = [(f"group:g{T[0]}#member@group:g{X[0]}#member", 100), (f"group:g{Y[-1]}#member@group:g{Z[-1]}#member", 200)]
    return g, ups, {0: set(), 150: {1, 10, 4, 7}, 250: {1, 10, 4, 7, 6, 5}}


def pyoracle_of(schema, g, ups, t0):
    """oracle/pyoracle.py over the same graph, by name"""
    from oracle import pyoracle
    py = pyoracle.PyOracle(schema)
    at = {r: t0 + d for r, d in ups}
    for p, c in g.nest:
        py.touch("group", f"g{p}", "member", "group", f"g{c}", "member", expires=at.get(f"group:g{p}#member@group:g{c}#member", 0))
    for gr, u in g.mem:
        py.touch("group", f"g{gr}", "member", "user", f"u{u}")
    for p, gr in g.pod_view:
        py.touch("pod", f"p{p}", "viewer", "group", f"g{gr}", "member")
    return py


def test_an_expiring_nesting_under_two_hop_rows(aclgpu, monkeypatch):
    """Two nestings under the two-hop rows of family(2, 4, 3) run out, and one comes back, with no write: every (pod, user) pair -- alone and in a 4 096-item
    batch -- at four clocks (before, after the first expiry, after both, set back between the two) equals both oracles, answers and error codes.  The rows are
    in use before the first crossing, and that crossing is a patch, not a rebuild (a nesting whose liveness changes drops the rows: plan.cpp "group nesting
    edited").  The dropped rows make a background build due: on this graph of 257 words it is adopted at the second crossing (the crossing replayed onto it), and
    the third finds more garbage than graph and rebuilds -- so from the second crossing on the test holds the snapshot to "followed the clock by a patch, an
    adopted build or a rebuild", never to which.  After the next rebuild the rows are back and the answers unchanged."""
    from oracle import pyoracle
    schema = _fuzz_tool().SCHEMA_C4_EXPIRING
    g, ups, lost = expiring_family()
    t0 = 1_700_000_000
    monkeypatch.delenv("ACL_HOP2", raising=False)
    o = orc.Oracle(schema)
    py = pyoracle_of(schema, g, ups, t0)
    res, subj = np.zeros(N_USER, dtype=np.uint32), np.arange(N_USER, dtype=np.uint32)
    with aclgpu.Engine(schema, device=0) as e:
        for x in (o, e):
            x.set_now(t0)
            g.load(x)
            x.write([(orc.OP_TOUCH, r, t0 + d) for r, d in ups])  # (re-written with an expiry behind the bulk load, before the first snapshot is built)

        def at(d, where):
            for x in (o, e):
                x.set_now(t0 + d)
            py.now = t0 + d
            perm, err = o.check_bulk_ids("pod", "view", res, "user", "", subj)
            want = np.array([u < 12 and u not in lost[d] for u in range(N_USER)])
            assert np.array_equal(perm == orc.PERM_HAS, want) and not err.any(), (where, perm)
            assert [py.check("pod", "p0", "view", "user", f"u{u}") == pyoracle.HAS for u in range(N_USER)] == want.tolist(), where
            for i in range(N_USER):
                p, er = e.check_bulk_ids(e.make_items("pod", "view", res[i:i + 1], "user", "", subj[i:i + 1]))
                assert p[0] == perm[i] and er[0] == err[i], (where, i, p, perm[i], er, err[i])
            k = np.arange(4096) % N_USER
            p, er = e.check_bulk_ids(e.make_items("pod", "view", res[k], "user", "", subj[k]))
            assert np.array_equal(p, perm[k]) and np.array_equal(er, err[k]), (where, np.flatnonzero(p != perm[k])[:8])
            return e.stats()

        st0 = at(0, "before")
        assert st0["hop2_rows"] > 0 and st0["local_passes"] > 0, st0
        st = at(150, "after the first expiry")
        assert st["snapshot_builds"] == st0["snapshot_builds"] and st["snapshot_patches"] > st0["snapshot_patches"], (st0, st)
        moves = lambda s_: s_["snapshot_builds"] + s_["snapshot_patches"] + s_["snapshot_compactions"]  # noqa: E731
        assert st["hop2_rows"] == 0, st  # (dropped with the patch)
        st2 = at(250, "after both")
        assert moves(st2) > moves(st), (st, st2)
        st = at(150, "set back between the two")
        assert moves(st) > moves(st2), (st2, st)
        assert st["expand_launches"] == 0 and st["overflow_retries"] == 0, st
        # a bulk load bypasses the change feed: the next read rebuilds -- at this clock, one nesting expired and one alive
        for x in (o, e):
            x.add_edges("pod", "creator", "user", "", u32([0]), u32([N_USER - 1]))
        py.touch("pod", "p0", "creator", "user", f"u{N_USER - 1}")
        lost[150] = lost[150] - {N_USER - 1}
        for x in (o, e):
            x.set_now(t0 + 150)
        perm, err = o.check_bulk_ids("pod", "view", res, "user", "", subj)
        assert perm[N_USER - 1] == orc.PERM_HAS and (perm[:12] == orc.PERM_HAS).tolist() == [u not in lost[150] for u in range(12)]
        k = np.arange(4096) % N_USER
        p, er = e.check_bulk_ids(e.make_items("pod", "view", res[k], "user", "", subj[k]))
        assert np.array_equal(p, perm[k]) and np.array_equal(er, err[k])
        st2 = e.stats()
        assert st2["snapshot_builds"] + st2["snapshot_compactions"] > st0["snapshot_builds"] + st0["snapshot_compactions"] and st2["hop2_rows"] > 0, (st0, st2)
    o.close()

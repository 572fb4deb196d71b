"""The seams of the reverse one-block walk (kernels.hip rev_block_walk, under k_rev_local and k_rev_multi): the reverse-direction counterpart of
tests/test_block_walk_seams_gpu.py -- graphs at the smallest sizes where an off-by-one in the shared skeleton shows.  One reverse row around a wave, a block
round and a trip of the row walk (U * 1 024 = 2 048 outputs); a level whose (state, op) pairs cross one round of 1 024 for W = 1, 2 and 3 parent ops per
slot; a log that ends one entry before, at and one entry behind its capacity; rounds at and around the size from which k_rev_local defers its terminal rows.

Every graph of a family lives in ONE engine as a component of its own, under a user of its own (a block walks one lookup: it sees its component only), and
every user is answered three ways -- single-target (k_rev_local), two targets with ACL_REV_MULTI_MIN_T=2 (k_rev_multi), and with ACL_REV_LOCAL=0 (the level
loop) -- each held to the C oracle's Check over every object of the target's type; the multi rows must also equal the single-target rows bit for bit.  So that
a fallback cannot hide a broken kernel, every lookup that is not meant to overflow asserts that its pass counter rose and `overflow_retries` did not.

The log's capacity: ACL_LOCAL_CAP has a floor of 256 entries (engine.cpp), so the log family walks 192 first visits in three levels of 64 before its level
of 63, 64 and 65: the log ends at 255, 256 and 257 entries, and by log_append's rule (base + count > cap stops) 256 fit and 257 do not."""
import numpy as np
import pytest

from oracle import orc
from tests.test_lookup_subjects_gpu import SCHEMA_BIG, ids_of

pytestmark = pytest.mark.gpu

PERM_HAS = 2
ROW_LENGTHS = [1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049]
LEVEL_WIDTHS = [340, 341, 342, 343, 511, 512, 513, 1023, 1024, 1025]
LOG_CAP = 256
LOG_LEVEL = [63, 64, 65]
DEFER_MIN = 64
TARGETS = [("pod", "view"), ("group", "member")]

# W = the most parent ops any slot has: group#member feeds pod#viewer (1), + group#member (2), + pod#editor (3)
SCHEMA_W = {
    1: "definition user {}\ndefinition group { relation member: user }\ndefinition pod {\n relation viewer: user | group#member\n permission view = viewer\n}",
    2: SCHEMA_BIG,
    3: "definition user {}\ndefinition group { relation member: user | group#member }\n"
       "definition pod {\n relation viewer: user | group#member\n relation editor: user | group#member\n permission view = viewer + editor\n}",
}


@pytest.fixture(scope="module")
def aclgpu(aclgpu_lib):
    import aclgpu as m
    return m


def u32(x):
    return np.asarray(x, dtype=np.uint32)


class Graph:
    """edges [(rtype, rel, stype, srel, res ids, subj ids)] over dense ids handed out per type; one user per case"""

    def __init__(self, schema):
        self.schema, self.edges, self.next = schema, [], {"user": 0, "group": 0, "pod": 0}

    def ids(self, t, n):
        a = np.arange(self.next[t], self.next[t] + n, dtype=np.uint32)
        self.next[t] += n
        return a

    def add(self, rt, rel, st, srel, r, s):
        self.edges.append((rt, rel, st, srel, u32(r), u32(s)))

    def member(self, groups, user):
        self.add("group", "member", "user", "", groups, np.full(len(groups), user, dtype=np.uint32))

    def own_pods(self, groups, rel="viewer"):
        """each group is `rel` of a pod of its own"""
        self.add("pod", rel, "group", "member", self.ids("pod", len(groups)), groups)

    def load(self, t):
        for rt, rel, st, srel, r, s in self.edges:
            t.add_edges(rt, rel, st, srel, r, s)

    def expected(self):
        """{user: {target: ids}} by the C oracle's Check over every object of the target's type (computed once, never modified)"""
        o = orc.Oracle(self.schema)
        self.load(o)
        out = {}
        for u in range(self.next["user"]):
            out[u] = {}
            for rt, pm in TARGETS:
                n = self.next[rt]
                p, err = o.check_bulk_ids_mt(8, rt, pm, np.arange(n, dtype=np.uint32), "user", "", np.full(n, u, dtype=np.uint32))
                assert not err.any()
                out[u][(rt, pm)] = set(np.flatnonzero(p == PERM_HAS).tolist())
        return out


def three_ways(aclgpu, monkeypatch, g, env=None, overflows=()):
    """every user of `g` by k_rev_local, k_rev_multi and the level loop, one lookup per call; users in `overflows` must send their walk to the fallback"""
    want = g.expected()
    users = list(range(g.next["user"]))
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    single = {}
    with aclgpu.Engine(g.schema, device=0) as e:  # ---- single-target: k_rev_local
        g.load(e)
        for u in users:
            for t in TARGETS:
                e.stats_reset()
                b, c = e.lookup_ids_batch(t[0], t[1], "user", "", u32([u]))
                st = e.stats()
                assert ids_of(b[0]) == want[u][t] and int(c[0]) == len(want[u][t]), (u, t)
                if u in overflows:
                    assert st["overflow_retries"] >= 1 and st["rev_local_passes"] == 0 and st["expand_launches"] > 0, (u, t, st)
                else:
                    assert st["rev_local_passes"] == 1 and st["overflow_retries"] == 0 and st["expand_launches"] == 0, (u, t, st)
                single[(u, t)] = b[0].copy()
    monkeypatch.setenv("ACL_REV_MULTI_MIN_T", "2")
    with aclgpu.Engine(g.schema, device=0) as e:  # ---- two targets: k_rev_multi
        g.load(e)
        for u in users:
            e.stats_reset()
            rows, counts = e.lookup_ids_multi(TARGETS, "user", "", u32([u]))
            st = e.stats()
            for j, t in enumerate(TARGETS):
                assert ids_of(rows[j][0]) == want[u][t] and int(counts[0, j]) == len(want[u][t]), (u, t)
                assert np.array_equal(rows[j][0], single[(u, t)]), (u, t)
            if u in overflows:
                assert st["overflow_retries"] >= 1 and st["rev_multi_passes"] == 0, (u, st)
            else:
                assert st["rev_multi_passes"] == 1 and st["overflow_retries"] == 0 and st["rev_local_passes"] == 0 and st["expand_launches"] == 0, (u, st)
    monkeypatch.delenv("ACL_REV_MULTI_MIN_T")
    monkeypatch.setenv("ACL_REV_LOCAL", "0")
    with aclgpu.Engine(g.schema, device=0) as e:  # ---- the level loop: k_rev_expand
        g.load(e)
        for t in TARGETS:
            e.stats_reset()
            b, c = e.lookup_ids_batch(t[0], t[1], "user", "", u32(users))
            st = e.stats()
            assert st["rev_local_passes"] == 0 and st["rev_multi_passes"] == 0 and st["expand_launches"] > 0, st
            for u in users:
                assert ids_of(b[u]) == want[u][t] and int(c[u]) == len(want[u][t]), (u, t)
                assert np.array_equal(b[u], single[(u, t)]), (u, t)
    return want


def test_row_length(aclgpu, monkeypatch):
    """one reverse row of n ids: user k is a member of n_k groups, each the viewer of a pod of its own"""
    g = Graph(SCHEMA_BIG)
    for n in ROW_LENGTHS:
        groups = g.ids("group", n)
        g.member(groups, g.ids("user", 1)[0])
        g.own_pods(groups)
    want = three_ways(aclgpu, monkeypatch, g)
    assert [len(want[u][("pod", "view")]) for u in sorted(want)] == ROW_LENGTHS


@pytest.mark.parametrize("W", [1, 2, 3])
def test_level_width(aclgpu, monkeypatch, W):
    """a level of g states whose slot has W parent ops: g * W pairs cross one round of 1 024"""
    g = Graph(SCHEMA_W[W])
    for n in LEVEL_WIDTHS:
        groups = g.ids("group", n)
        g.member(groups, g.ids("user", 1)[0])
        g.own_pods(groups)
        if W == 3:
            g.own_pods(groups[::2], "editor")
    want = three_ways(aclgpu, monkeypatch, g)
    assert [len(want[u][("pod", "view")]) for u in sorted(want)] == [n + (n + 1) // 2 if W == 3 else n for n in LEVEL_WIDTHS]


def test_log_end(aclgpu, monkeypatch):
    """a log of LOG_CAP entries that ends at 255, 256 and 257 first visits: three levels of 64 nested groups, then a level of 63, 64 and 65 (whose pods are
    terminal children and never logged)"""
    g = Graph(SCHEMA_BIG)
    for n in LOG_LEVEL:
        level = g.ids("group", 64)
        g.member(level, g.ids("user", 1)[0])
        for width in (64, 64, n):
            above = g.ids("group", width)
            g.add("group", "member", "group", "member", above, level[np.arange(width) % 64])  # (the 65th group sits above the first of the level below)
            level = above
        g.own_pods(level)
    want = three_ways(aclgpu, monkeypatch, g, env={"ACL_LOCAL_CAP": str(LOG_CAP)}, overflows={2})
    assert [len(want[u][("pod", "view")]) for u in sorted(want)] == LOG_LEVEL
    assert [len(want[u][("group", "member")]) for u in sorted(want)] == [LOG_CAP - 64 + n for n in LOG_LEVEL]


def test_deferral(aclgpu, monkeypatch):
    """k_rev_local with the result rows in HBM defers the terminal rows of a round of DEFER_MIN children or more: one group that is the viewer of 63, 64 and
    65 pods; and a round that 70 deferred children share with a row of another slot (the group's 5 parent groups, each the viewer of a pod of its own), so the
    scan behind the deferral runs with a remainder of 5"""
    g = Graph(SCHEMA_BIG)
    for n, parents in [(63, 0), (64, 0), (65, 0), (70, 5)]:
        grp = g.ids("group", 1)
        g.member(grp, g.ids("user", 1)[0])
        g.add("pod", "viewer", "group", "member", g.ids("pod", n), np.full(n, grp[0], dtype=np.uint32))
        if parents:
            above = g.ids("group", parents)
            g.add("group", "member", "group", "member", above, np.full(parents, grp[0], dtype=np.uint32))
            g.own_pods(above)
    want = three_ways(aclgpu, monkeypatch, g, env={"ACL_REV_LDS_ROWS": "0", "ACL_REV_DEFER_MIN": str(DEFER_MIN)})
    assert [len(want[u][("pod", "view")]) for u in sorted(want)] == [63, 64, 65, 75]

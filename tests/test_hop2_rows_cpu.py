"""Two-hop rows of nested groups (plan.hpp Snapshot::hop2_*) on store-only engines: which rows the builder composes (at least one grandchild,
children + grandchildren <= 16), that verify_snapshot accepts them (acl_selfcheck_snapshot checks every descriptor against the one-hop rows it was
composed from), and that the patcher keeps them under writes to every other class and DROPS them -- never patches them -- when group nesting or a
group's leaf status changes.  The walk that reads them is covered by tests/test_hop2_walk_gpu.py."""
import numpy as np
import pytest

from aclgpu import workloads
from aclgpu.workloads import SCHEMA_C4

CAP = 16


@pytest.fixture(scope="module")
def aclgpu(aclgpu_lib):
    import aclgpu as m
    return m


def u32(a):
    return np.asarray(a, dtype=np.uint32)


def two_hop_count(gr, gs):
    """the numpy composition: groups with >= 1 grandchild and children + distinct grandchildren <= CAP"""
    kids = {}
    for r, s in zip(gr.tolist(), gs.tolist()):
        kids.setdefault(r, set()).add(s)
    n = 0
    for g, ch in kids.items():
        gc = set()
        for c in ch:
            gc |= kids.get(c, set())
        n += bool(gc) and len(ch) + len(gc) <= CAP
    return n


def engine_of(aclgpu, nest, n_group, extra=()):
    """store-only engine over SCHEMA_C4: groups g0.., users u0..u7, pod p0, namespace n0 interned in id order; nest = [(parent, child)]"""
    e = aclgpu.Engine(SCHEMA_C4, store_only=True)
    for i in range(n_group):
        assert e.intern("group", f"g{i}") == i
    for k in range(8):
        assert e.intern("user", f"u{k}") == k
    assert e.intern("pod", "p0") == 0 and e.intern("namespace", "n0") == 0
    if nest:
        e.add_edges("group", "member", "group", "member", u32([p for p, _ in nest]), u32([c for _, c in nest]))
    e.add_edges("pod", "viewer", "group", "member", u32([0]), u32([0]))
    e.add_edges("group", "member", "user", "", u32([n_group - 1]), u32([0]))
    for ed in extra:
        e.add_edges(*ed)
    return e


def tree(a, gc_total):
    """g0 with `a` children g1..ga and gc_total distinct grandchildren spread over them -> (nest, n_group)"""
    nest = [(0, 1 + i) for i in range(a)]
    nest += [(1 + k % a, 1 + a + k) for k in range(gc_total)]
    return nest, 1 + a + gc_total


def test_c4_rows_match_the_numpy_composition(aclgpu):
    w = workloads.c4(scale=0.01, batch=64)
    (gr, gs), = [(ed[4], ed[5]) for ed in w.edges if ed[:4] == ("group", "member", "group", "member")]
    want = two_hop_count(gr, gs)
    assert want > 100
    e = aclgpu.Engine(w.schema, store_only=True)
    w.load(e)
    assert e.selfcheck_snapshot_code() == 0
    assert e.stats()["hop2_rows"] == want
    e.close()


@pytest.mark.parametrize("a,gc,rows", [(4, 12, 1), (4, 13, 0), (1, 1, 1), (15, 1, 1), (15, 2, 0), (16, 1, 0), (3, 0, 0)])
def test_the_cap_and_the_rows_without_grandchildren(aclgpu, a, gc, rows):
    """a row of exactly 16 ids is two-hop, one of 17 is not; a group whose children are all leaves keeps its one-hop descriptor (the children g1..ga of
    every tree here are such groups: only g0 can have a two-hop row)"""
    nest, ng = tree(a, gc)
    e = engine_of(aclgpu, nest, ng)
    assert e.selfcheck_snapshot_code() == 0
    assert e.stats()["hop2_rows"] == rows
    e.close()


def test_an_id_that_is_child_and_grandchild_counts_twice(aclgpu):
    # g0 -> g1..g8; g1 -> g2..g8 (7 grandchildren that are children too) = 15; one more grandchild g9 = 16; with g10 as well = 17
    base = [(0, i) for i in range(1, 9)] + [(1, i) for i in range(2, 9)]
    for extra, rows in (([(1, 9)], 1), ([(1, 9), (1, 10)], 0)):
        e = engine_of(aclgpu, base + extra, 12)
        assert e.selfcheck_snapshot_code() == 0
        assert e.stats()["hop2_rows"] == rows
        e.close()


def test_cycles_build_and_verify(aclgpu):
    for nest, ng, rows in (([(0, 1), (1, 0)], 3, 2), ([(0, 0)], 2, 1), ([(0, 1), (1, 2), (2, 0)], 4, 3)):
        e = engine_of(aclgpu, nest, ng)
        assert e.selfcheck_snapshot_code() == 0
        assert e.stats()["hop2_rows"] == rows
        e.close()


def test_writes_keep_or_drop_the_rows(aclgpu):
    # g0 -> g1, g2; g1 -> g3, g4; g2 -> g4, g5; g3 -> g6; g7 and g8 are leaves outside the tree (g8 holds u0)
    nest = [(0, 1), (0, 2), (1, 3), (1, 4), (2, 4), (2, 5), (3, 6)]
    e = engine_of(aclgpu, nest, 9)
    rows = two_hop_count(u32([p for p, _ in nest]), u32([c for _, c in nest]))
    assert rows == 2  # g0 and g1

    def count():
        return two_hop_count(u32([p for p, _ in nest]), u32([c for _, c in nest]))

    def rebuilt():
        # a bulk load bypasses the change feed: the next read rebuilds, and the rows are back
        e.add_edges("pod", "creator", "user", "", u32([0]), u32([1]))
        assert e.selfcheck_snapshot_code() == 0
        assert e.stats()["hop2_rows"] == count() > 0

    def step(op, rel, want_rows):
        e.write([(op, rel)])
        assert e.selfcheck_snapshot_code() == 1, rel  # patched, not rebuilt (and verified against the store)
        assert e.stats()["hop2_rows"] == want_rows, rel

    assert e.selfcheck_snapshot_code() == 0 and e.stats()["hop2_rows"] == rows
    step(aclgpu.OP_TOUCH, "pod:p0#viewer@user:u3", rows)
    step(aclgpu.OP_TOUCH, "pod:p0#viewer@group:g7#member", rows)
    step(aclgpu.OP_TOUCH, "namespace:n0#viewer@group:g1#member", rows)
    step(aclgpu.OP_TOUCH, "group:g4#member@user:u2", rows)
    step(aclgpu.OP_DELETE, "group:g4#member@user:u2", rows)
    step(aclgpu.OP_TOUCH, "group:g5#member@group:g6#member", 0)  # nesting added (g5 was a leaf: its flags are distrusted as well)
    step(aclgpu.OP_TOUCH, "group:g4#member@user:u5", 0)           # ... and they stay dropped until a build
    nest.append((5, 6))
    rebuilt()
    assert count() == 3  # g0, g1 and now g2 (g5 -> g6)
    step(aclgpu.OP_DELETE, "group:g3#member@group:g6#member", 0)  # nesting deleted
    nest.remove((3, 6))
    rebuilt()
    step(aclgpu.OP_TOUCH, "group:g0#member@group:g7#member", 0)  # a row that already had children grows
    nest.append((0, 7))
    rebuilt()
    step(aclgpu.OP_TOUCH, "group:g7#member@group:g8#member", 0)  # a leaf group stops being one
    nest.append((7, 8))
    rebuilt()
    e.close()


def test_an_expiry_drops_the_rows_with_a_patch_and_a_build_brings_them_back(aclgpu):
    """The host half of tests/test_hop2_walk_gpu.py test_an_expiring_nesting_under_two_hop_rows: a nesting under a two-hop row runs out (and comes back when
    the clock is set back) with no write -- the snapshot follows by a patch that drops the rows, verified against the store at every clock; a build at a clock
    between the two expiries composes rows over the live nestings again."""
    from tests.test_hop2_walk_gpu import N_USER, _fuzz_tool, expiring_family
    g, ups, _lost = expiring_family()
    t0 = 1_700_000_000
    e = aclgpu.Engine(_fuzz_tool().SCHEMA_C4_EXPIRING, store_only=True)
    e.set_now(t0)
    g.load(e)
    e.write([(aclgpu.OP_TOUCH, r, t0 + d) for r, d in ups])
    assert e.selfcheck_snapshot_code() == 0
    rows = e.stats()["hop2_rows"]
    assert rows == two_hop_count(u32([p for p, _ in g.nest]), u32([c for _, c in g.nest])) > 0
    e.set_now(t0 + 50)
    assert e.selfcheck_snapshot_code() == 2 and e.stats()["hop2_rows"] == rows  # (nothing crossed: current)
    for d in (150, 250, 150):
        e.set_now(t0 + d)
        assert e.selfcheck_snapshot_code() == 1 and e.stats()["hop2_rows"] == 0, d  # patched, verified against the store; the rows are dropped
    e.add_edges("pod", "creator", "user", "", u32([0]), u32([N_USER - 1]))
    assert e.selfcheck_snapshot_code() == 0
    live = [(p, c) for p, c in g.nest if (p, c) != (0, 2)]  # (T[0] -> X[0] is expired at +150 s)
    assert e.stats()["hop2_rows"] == two_hop_count(u32([p for p, _ in live]), u32([c for _, c in live])) > 0
    e.close()

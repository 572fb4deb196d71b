"""The seams of the helpers the one-block walks share (kernels.hip block_excl_scan, log_append, task_owner, subj_decode, subj_block_walk; the host's
block_walk_chunks): graphs at the smallest sizes where an off-by-one in one of them shows -- a row around a wave, a block round and two rounds of the row
walk; a level whose (state, op) pairs cross one round of 1 024 for 1, 2 and 3 ops per state; a level around the first log region of 2^14 entries.

Every graph is answered four ways, each against the expected value (the C oracle's Check over every user; the log-region graphs give theirs in closed form):
LookupSubjects by the one-block kernel (k_subj_local), LookupSubjects by the level loop (k_subj_expand: a sharded engine of world 1), Explain for the last
user of the row (k_explain_local; the witness goes through tests/explain_checker.py) and LookupResources from that user (k_rev_local)."""
import functools

import numpy as np
import pytest

from oracle import orc
from tests import explain_checker as X
from tests.test_explain_gpu import namer
from tests.test_lookup_subjects_gpu import SCHEMA_BIG, check_rows, ids_of
from tests.test_sharded_subjects_gpu import rows_of, run_shards

pytestmark = pytest.mark.gpu

PERM_HAS = 2
ROW_LENGTHS = [1, 63, 64, 65, 1023, 1024, 1025, 2049]
LEVEL_WIDTHS = [340, 341, 342, 343, 511, 512, 513, 1023, 1024, 1025]
LOG_REGION = [16382, 16383, 16384, 16385]  # (the first region holds 2^14 entries and the root takes one)


@pytest.fixture(scope="module")
def aclgpu(aclgpu_lib):
    import aclgpu as m
    return m


def u32(x):
    return np.asarray(x, dtype=np.uint32)


def row_graph(n):
    """pod 0 <- group 0 <- users 0 .. n-1: one row of n ids"""
    return [("pod", "viewer", "group", "member", u32([0]), u32([0])), ("group", "member", "user", "", np.zeros(n, dtype=np.uint32), np.arange(n, dtype=np.uint32))]


def wide_graph(g):
    """pod 0 <- groups 0 .. g-1, group k <- user k: a level of g states"""
    ks = np.arange(g, dtype=np.uint32)
    return [("pod", "viewer", "group", "member", np.zeros(g, dtype=np.uint32), ks), ("group", "member", "user", "", ks, ks)]


def load(t, edges):
    for rt, rel, st, srel, r, s in edges:
        t.add_edges(rt, rel, st, srel, r, s)


@functools.lru_cache(maxsize=None)
def oracle_row(kind, n):
    """pod 0's expected row by the C oracle's Check over every user (computed once per graph, shared, never modified)"""
    o = orc.Oracle(SCHEMA_BIG)
    load(o, row_graph(n) if kind == "row" else wide_graph(n))
    return frozenset(check_rows(o, "pod", "view", u32([0]), "user", "", n)[0])


def four_paths(aclgpu, edges, want, last):
    """pod 0's users by both LookupSubjects kernels, the witness of (pod 0, view, user `last`) and the pods of user `last`"""
    stored = set()
    for rt, rel, st, srel, r, s in edges:
        stored.update((rt, str(int(a)), rel, st, str(int(b)), srel) for a, b in zip(r, s))
    with aclgpu.Engine(SCHEMA_BIG, device=0) as e:
        load(e, edges)
        bms, counts, flags = e.lookup_subjects_ids_batch("pod", "view", "user", "", u32([0]))
        assert ids_of(bms[0]) == want and int(counts[0]) == len(want) and flags[0] == 0
        items = e.make_items("pod", "view", [0], "user", "", [last])
        perm, err, xflags, off, raw = e.explain_ids(items)
        assert (int(perm[0]), int(err[0]), int(xflags[0])) == (PERM_HAS, 0, aclgpu.EXPLAIN_WITNESS)
        hops = namer(e, SCHEMA_BIG, named=False)(raw)
        assert len(hops) == 2 and off.tolist() == [0, 2]  # pod <- group <- user
        X.check_witness(SCHEMA_BIG, stored, ("pod", "0", "view", "user", str(last), ""), hops)
        e.stats_reset()
        pods, pcounts = e.lookup_ids_batch("pod", "view", "user", "", u32([last]))
        st = e.stats()
        assert st["rev_local_passes"] == 1 and st["expand_launches"] == 0  # (the single launch answered, as tests/test_lookup_local_gpu.py asserts it)
        assert ids_of(pods[0]) == {0} and int(pcounts[0]) == 1

    def run(se):
        b, f, _x, _s = se.lookup_subjects_ids_batch_native("pod", "view", "user", "", u32([0]))
        return rows_of(b), f

    (b, f), = run_shards(aclgpu, 1, SCHEMA_BIG, lambda e: load(e, edges), run)
    assert ids_of(b[0]) == want and not f.any()


@pytest.mark.parametrize("n", ROW_LENGTHS)
def test_row_length(aclgpu, n):
    """one row of n ids: a wave, one round of the row walk, two rounds, and the word seams of the fold that marks ascending ids"""
    want = oracle_row("row", n)
    assert want == frozenset(range(n))
    four_paths(aclgpu, row_graph(n), want, n - 1)


@pytest.mark.parametrize("g", LEVEL_WIDTHS)
def test_level_width(aclgpu, g):
    """a level of g states: g * W pairs cross one round of 1 024 for W = 3, 2 and 1 ops per state (the engine does not expose W: every size runs)"""
    want = oracle_row("wide", g)
    assert want == frozenset(range(g))
    four_paths(aclgpu, wide_graph(g), want, g - 1)


@pytest.mark.parametrize("g", LOG_REGION)
def test_log_region(aclgpu, g):
    """g groups under one pod, at and around the size where the first attempt's log overflows and the driver walks again: the row is the groups' members
    (user k of group k: the closed form, as the 20 000-group case of tests/test_lookup_subjects_gpu.py)"""
    four_paths(aclgpu, wide_graph(g), frozenset(range(g)), g - 1)


def test_mixed_batch(aclgpu):
    """1 025 lookups in one call, the pod of the 1 025-long row among pods without relationships: every row equals its single lookup's"""
    n = 1025
    want = oracle_row("row", n)
    with aclgpu.Engine(SCHEMA_BIG, device=0) as e:
        load(e, row_graph(n))
        empty = [e.intern("pod", f"no-relationships-{k}") for k in range(7)]
        rids = u32([empty[i % 7] for i in range(n)])
        full = [0, 1, 63, 64, 511, 512, 1023, 1024]
        rids[full] = 0
        bms, counts, flags = e.lookup_subjects_ids_batch("pod", "view", "user", "", rids)
        single = {int(r): e.lookup_subjects_ids_batch("pod", "view", "user", "", u32([r])) for r in [0] + empty}
        assert ids_of(single[0][0][0]) == want
        for i, r in enumerate(rids):
            b1, c1, f1 = single[int(r)]
            assert np.array_equal(bms[i], b1[0]) and counts[i] == c1[0] and flags[i] == f1[0], i
            assert bool(bms[i].any()) == (i in full)

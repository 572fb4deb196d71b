"""The single-launch walk's deep levels at every pair and step boundary, equal to the oracle item by item (kernels.hip: k_check_local's claim
loop, process_segment's direct form, simple_steps).

The graph family (SCHEMA_C4): one pod viewed by group A; A contains n groups B_1..B_n; every B_j contains d leaf groups C_jk that hold users.
A `pod#view@user` request then walks pod -> A -> the B's -> the C's: its third level is exactly n entries -- probed, plain-subject states of ONE
slot -- whose pairs of segments expand to n d children on the direct form.  What the shapes cover:
  - n odd and even, one segment, one pair, several pairs and every boundary of 64 and 128 entries (segments are claimed in pairs; the level's last
    loads are clamped);
  - n d on every residue of 64 and of 192: the last step of an expansion is one, two or three windows of 64 children wide;
  - subjects whose only membership is the C at the first work item, at the first lane of the last pair's last window and at its last valid lane,
    and a subject that is a member of nothing;
  - a 1-item batch (the items ride in the launch's arguments, narrow blocks), a 4 096-item batch that mixes every subject in one unit, and for
    n in {65, 129, 193} a 65 536-item batch (the 12-wave blocks).
Then the row descriptors the walk keeps per request (k_check_local's s_sd): subjects with and without a row of the hot hashed class, the user with
the highest id, userset subjects (another subject key: the generic path), all in one unit; and a user's hashed row re-placed by the patcher between
two batches.  (SCHEMA_C4 has no second plain subject type on `viewer`, so there is no plain subject of another key.)"""
import numpy as np
import pytest

from aclgpu.workloads import SCHEMA_C4
from oracle import orc

pytestmark = pytest.mark.gpu

SHAPES = [(n, 1) for n in (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 257, 384, 385)] + [(100, 3), (128, 4)]
WIDE = (65, 129, 193)
N_USER = 64          # users 0..7 are the placed ones, N_USER - 1 is the highest id of the type; the rest have no relationship
U_FIRST, U_LAST, U_HEAD, U_ALL, U_NONE, U_TOP = 0, 1, 2, 5, 6, N_USER - 1


@pytest.fixture(scope="module")
def aclgpu(aclgpu_lib):
    import aclgpu as m
    return m


def _children(n, d):
    """-> (c_of [n, d] ids of the C groups under B_1..B_n, last): the C's of the level's LAST pair of segments in work-item order"""
    c_of = (1 + n + np.arange(n * d)).reshape(n, d)
    base = 128 * ((n - 1) // 128)
    return c_of, c_of[np.arange(base, n)].reshape(-1)


def _graph(n, d):
    """-> edges.  group ids: A = 0, B_j = j (1..n), C_jk = 1 + n + (j - 1) d + k"""
    c_of, level = _children(n, d)
    total = level.size
    head, last = 64 * ((total - 1) // 64), total - 1
    u32 = lambda a: np.asarray(a, dtype=np.uint32)  # noqa: E731
    allc = c_of.reshape(-1)
    mem = [(c_of[0, 0], U_FIRST), (level[last], U_LAST), (level[head], U_HEAD), (c_of[n // 2, d - 1], U_TOP)]
    gr = np.concatenate([[g for g, _ in mem], allc])
    gs = np.concatenate([[u for _, u in mem], np.full(allc.size, U_ALL)])
    return [("pod", "viewer", "group", "member", u32([0]), u32([0])),
            ("group", "member", "group", "member", u32(np.concatenate([np.zeros(n), np.repeat(1 + np.arange(n), d)])), u32(np.concatenate([1 + np.arange(n), allc]))),
            ("group", "member", "user", "", u32(gr), u32(gs))]


def _intern(target, n, d):
    """names in id order, so that writes by name meet the numeric ids (user "u<k>" = k, group "g<i>" = i, pod "p0" = 0)"""
    for k in range(N_USER):
        assert target.intern("user", f"u{k}") == k
    for i in range(1 + n + n * d):
        assert target.intern("group", f"g{i}") == i
    assert target.intern("pod", "p0") == 0


def _load(target, n, d):
    _intern(target, n, d)
    for rt, rel, st, sr, res, subj in _graph(n, d):
        target.add_edges(rt, rel, st, sr, res, subj)


def _mixed(e, o, n, size):
    """-> (items, oracle perm, oracle err) of `size` items: every kind of subject, interleaved so that one unit holds them all"""
    users = np.array([U_FIRST, U_LAST, U_HEAD, U_ALL, U_NONE, U_TOP, 7, 33], dtype=np.uint32)
    sets = np.array([0, 1, n, 1 + n, min(2, n)], dtype=np.uint32)  # group:<id>#member: A itself, B_1, B_n, a C, B_2
    k = np.arange(size)
    is_set = k % 5 == 4
    sub = np.where(is_set, sets[(k // 5) % sets.size], users[(k - k // 5) % users.size]).astype(np.uint32)
    res = np.zeros(size, dtype=np.uint32)
    items = e.make_items("pod", "view", res, "user", "", sub)
    items[is_set] = e.make_items("pod", "view", res[is_set], "group", "member", sub[is_set])
    op, oe = np.zeros(size, dtype=np.uint8), np.zeros(size, dtype=np.int32)
    op[~is_set], oe[~is_set] = o.check_bulk_ids("pod", "view", res[~is_set], "user", "", sub[~is_set])
    op[is_set], oe[is_set] = o.check_bulk_ids("pod", "view", res[is_set], "group", "member", sub[is_set])
    return items, op, oe


def _oracle_shape(o, n):
    """the oracle side of the graph: who holds pod:0#view"""
    users = np.arange(N_USER, dtype=np.uint32)
    op, oe = o.check_bulk_ids("pod", "view", np.zeros(N_USER, dtype=np.uint32), "user", "", users)
    want = np.zeros(N_USER, dtype=bool)
    want[[U_FIRST, U_LAST, U_HEAD, U_ALL, U_TOP]] = True
    assert np.array_equal(op == orc.PERM_HAS, want) and np.array_equal(op == orc.PERM_NO, ~want) and not oe.any(), (n, op)


@pytest.mark.parametrize("n,d", SHAPES)
def test_pairs_and_last_steps(n, d, aclgpu):
    o = orc.Oracle(SCHEMA_C4)
    _load(o, n, d)
    _oracle_shape(o, n)
    with aclgpu.Engine(SCHEMA_C4, device=0) as e:
        _load(e, n, d)
        e.stats_reset()
        zero = np.zeros(1, dtype=np.uint32)
        for u in (U_FIRST, U_LAST, U_HEAD, U_ALL, U_NONE, U_TOP):  # 1-item batches
            p, er = e.check_bulk_ids(e.make_items("pod", "view", zero, "user", "", np.array([u], dtype=np.uint32)))
            op, oe = o.check_bulk_ids("pod", "view", zero, "user", "", np.array([u], dtype=np.uint32))
            assert np.array_equal(p, op) and np.array_equal(er, oe), (n, d, u, p, op, er, oe)
        sizes = (4096, 65536) if (d == 1 and n in WIDE) else (4096,)
        for size in sizes:
            items, op, oe = _mixed(e, o, n, size)
            assert (op == orc.PERM_HAS).any() and (op == orc.PERM_NO).any()
            p, er = e.check_bulk_ids(items)
            assert np.array_equal(p, op) and np.array_equal(er, oe), (n, d, size, int((p != op).sum()), int((er != oe).sum()), np.flatnonzero(p != op)[:8])
        st = e.stats()
        # the single-launch walk answered every batch itself: one that outgrew its private frontier, or its direct task lists, is redone on the level loop
        assert st["local_passes"] >= 7 and st["expand_launches"] == 0 and st["overflow_retries"] == 0, st


def test_row_replaced_by_the_patcher(aclgpu):
    """U_NONE has no row of group#member@user, user 7 none either; a write gives user 7 forty memberships (its row is placed anew, with more buckets) and
    U_LAST thirty more (its one-bucket row moves): the batches before and after equal the oracle, and the write was a patch of the device snapshot"""
    n, d = 100, 3
    o = orc.Oracle(SCHEMA_C4)
    _load(o, n, d)
    c_of, _level = _children(n, d)
    far = np.arange(n * d + n + 1, n * d + n + 1 + 40)  # forty new groups outside the pod's tree ...
    ups = [("group", f"g{int(g)}", "member", "user", "u7", "") for g in far[:39]] + [("group", f"g{int(c_of[n - 1, d - 1])}", "member", "user", "u7", "")]  # ... and the last C
    ups += [("group", f"g{int(g)}", "member", "user", f"u{U_LAST}", "") for g in far[:30]]
    with aclgpu.Engine(SCHEMA_C4, device=0) as e:
        _load(e, n, d)
        for t in (e, o):
            for g in far:
                assert t.intern("group", f"g{int(g)}") == int(g)
        items, op, oe = _mixed(e, o, n, 4096)
        p, er = e.check_bulk_ids(items)
        assert np.array_equal(p, op) and np.array_equal(er, oe)
        st0 = e.stats()
        e.write([(aclgpu.OP_TOUCH, r) for r in ups])
        o.write([(orc.OP_TOUCH, r) for r in ups])
        items, op2, oe2 = _mixed(e, o, n, 4096)
        assert (op2 != op).any()  # user 7 holds the permission now
        p, er = e.check_bulk_ids(items)
        assert np.array_equal(p, op2) and np.array_equal(er, oe2), (int((p != op2).sum()), np.flatnonzero(p != op2)[:8])
        st = e.stats()
        assert st["snapshot_builds"] == st0["snapshot_builds"] and st["snapshot_patches"] > st0["snapshot_patches"], (st0, st)

"""Watch sets: the refusals include/aclgpu.h lists that need a real set (a store-only engine never has one), acl_close with sets still open, and the
layer above the C ABI -- client.run_watch_set, the ONE poll loop of a set, with two watchers whose changes must both arrive."""
import ctypes as C

import numpy as np
import pytest

from oracle import orc

pytestmark = pytest.mark.gpu

OP_TOUCH, OP_DELETE = 2, 3
SCHEMA = """
definition user {}
definition namespace {
  relation viewer: user
  permission view = viewer
}
definition pod {
  relation namespace: namespace
  relation viewer: user
  permission view = viewer + namespace->view
}
"""


@pytest.fixture(scope="module")
def aclgpu(aclgpu_lib):
    import aclgpu as m
    return m


def code_of(aclgpu, call):
    with pytest.raises(aclgpu.AclError) as ei:
        call()
    return ei.value.code


def test_unknown_and_removed_watchers_and_short_rows_are_refused(aclgpu, aclgpu_lib):
    L = aclgpu_lib
    with aclgpu.Engine(SCHEMA, device=0) as e:
        e.write([(OP_TOUCH, ("pod", f"a/p{i}", "viewer", "user", "u0", "")) for i in range(70)])  # 70 pods: a row needs 3 words
        ws = e.watch_set("pod", "view", "user")
        w0, w1 = ws.add("u0"), ws.add("u1")
        # an id never issued
        assert code_of(aclgpu, lambda: ws.remove(7)) == aclgpu.ERR_INVALID_ARGUMENT
        assert code_of(aclgpu, lambda: ws.row(7)) == aclgpu.ERR_INVALID_ARGUMENT
        assert ws.row(w0).size == 0  # (added, not polled yet: the empty row, whatever the buffer)
        _rev, recs = ws.poll()
        assert recs.size == 70 and ws.row(w0).tolist() == list(range(70))
        # a row buffer below the need (3 words): refused, nothing written
        bm = np.full(4, 0xDEADBEEF, dtype=np.uint32)
        for words in (0, 1, 2):
            assert L.acl_watch_set_row(e._h, ws._s, w0, bm.ctypes.data, words) == aclgpu.ERR_INVALID_ARGUMENT
            assert b"bitmap too small" in L.acl_last_error() and (bm == 0xDEADBEEF).all()
        assert L.acl_watch_set_row(e._h, ws._s, w0, bm.ctypes.data, 3) == 0 and bm[:3].tolist() == [0xFFFFFFFF, 0xFFFFFFFF, 0x3F] and bm[3] == 0xDEADBEEF
        assert L.acl_watch_set_row(e._h, ws._s, w0, bm.ctypes.data, 4) == 0 and bm[3] == 0  # (the rest of a longer buffer is zeroed)
        # a removed watcher: its id is gone for good (ids are not reused), the other one's row moved up and is still its own
        ws.remove(w0)
        assert code_of(aclgpu, lambda: ws.remove(w0)) == aclgpu.ERR_INVALID_ARGUMENT
        assert code_of(aclgpu, lambda: ws.row(w0)) == aclgpu.ERR_INVALID_ARGUMENT
        e.write([(OP_TOUCH, ("pod", "a/p69", "viewer", "user", "u1", ""))])
        _rev, recs = ws.poll()
        assert [(int(r["watcher"]), int(r["resource_id"]), int(r["gained"])) for r in recs] == [(w1, 69, 1)] and ws.row(w1).tolist() == [69]
        assert ws.add("u2") == 2  # (not w0's number again)
        # unknown flags, an ill-formed subject id
        w = C.c_uint32()
        assert L.acl_watch_set_add(e._h, ws._s, b"u3", 2, C.byref(w)) == aclgpu.ERR_INVALID_ARGUMENT
        assert L.acl_watch_set_add(e._h, ws._s, b"not an id", 0, C.byref(w)) == aclgpu.ERR_INVALID_ARGUMENT
        ws.close()
        assert L.acl_watch_set_stats(e._h, ws._s if ws._s else C.c_void_p(0x1000), None, None, None) == aclgpu.ERR_INVALID_ARGUMENT


def test_a_sharded_engine_refuses_watch_sets(aclgpu, aclgpu_lib):
    with aclgpu.Engine(SCHEMA, device=0) as e:
        e.write([(OP_TOUCH, ("pod", "a/p0", "viewer", "user", "u0", ""))])
        before = e.watch_set("pod", "view", "user")  # opened while the engine still is one whole graph
        before.add("u0")
        assert before.poll()[1].size == 1
        e._check(aclgpu_lib.acl_shard_configure(e._h, 0, 2))
        assert code_of(aclgpu, lambda: e.watch_set("pod", "view", "user")) == aclgpu.ERR_FAILED_PRECONDITION
        e.write([(OP_TOUCH, ("pod", "a/p1", "viewer", "user", "u0", ""))])
        assert code_of(aclgpu, before.poll) == aclgpu.ERR_FAILED_PRECONDITION  # ... and a set from before does not evaluate on one shard
        assert before.row(0).tolist() == [0]  # (the baseline as it was)
        e._check(aclgpu_lib.acl_shard_configure(e._h, 0, 1))
        assert [int(r["resource_id"]) for r in before.poll()[1]] == [1]  # whole again: the difference against that baseline


def test_more_than_a_gibibyte_of_rows_is_refused_at_add(aclgpu):
    """2^25 pod ids (one bulk-loaded edge names the last one): a row is 4 MiB, the set's two arrays 8 MiB per watcher -- the 129th add would pass 1 GiB.
    Nothing is allocated on the device before a poll, so the adds themselves cost nothing."""
    with aclgpu.Engine(SCHEMA, device=0) as e:
        e.add_edges("pod", "viewer", "user", "", np.array([(1 << 25) - 1], dtype=np.uint32), np.array([0], dtype=np.uint32))
        assert e.object_count("pod") == 1 << 25
        ws = e.watch_set("pod", "view", "user")
        for i in range(128):
            assert ws.add(f"w{i}") == i
        assert code_of(aclgpu, lambda: ws.add("one-too-many")) == aclgpu.ERR_RESOURCE_EXHAUSTED
        ws.remove(5)
        assert ws.add("fits-again") == 128
        assert code_of(aclgpu, lambda: ws.add("one-too-many")) == aclgpu.ERR_RESOURCE_EXHAUSTED


def test_closing_the_engine_releases_open_sets(aclgpu):
    e = aclgpu.Engine(SCHEMA, device=0)
    e.write([(OP_TOUCH, ("pod", f"a/p{i}", "viewer", "user", "u0", "")) for i in range(40)])
    sets = [e.watch_set("pod", "view", "user") for _ in range(3)]
    for ws in sets[:2]:
        ws.add("u0")
        assert ws.poll()[1].size == 40  # (rows on the device, scratch arrays: what close has to free)
    e.close()  # two polled sets and one empty one still open
    for ws in sets:
        ws.close()  # (the handle went with the engine: nothing to do, nothing touched)
    with aclgpu.Engine(SCHEMA, device=0) as e2:  # the device is as usable as before
        e2.write([(OP_TOUCH, ("pod", "a/p0", "viewer", "user", "u0", ""))])
        ws = e2.watch_set("pod", "view", "user")
        ws.add("u0")
        assert ws.poll()[1].size == 1


def test_one_poll_loop_serves_every_watcher_of_the_set(aclgpu):
    """client.run_watch_set with two watchers: a namespace grant to each, written before ONE poll -- both watchers' changes arrive (through their
    sinks and in the loop's own stream), against the oracle's lookups; a second loop on the same set is refused while the first is open."""
    from aclgpu import client
    o = orc.Oracle(SCHEMA)
    with aclgpu.Engine(SCHEMA, device=0) as e:
        ups = [(OP_TOUCH, ("pod", f"{'ab'[i % 2]}/p{i}", "namespace", "namespace", "ab"[i % 2], "")) for i in range(20)]
        e.write(ups)
        o.write(ups)
        ws = e.watch_set("pod", "view", "user")
        wa, wb = ws.add("ua", from_now=True), ws.add("ub", from_now=True)
        got = {wa: [], wb: []}
        sinks = {wa: lambda allowed, oid: got[wa].append((allowed, oid)), wb: lambda allowed, oid: got[wb].append((allowed, oid))}
        assert list(client.run_watch_set(e, ws, sinks, polls=1)) == []  # the baseline
        ups = [(OP_TOUCH, ("namespace", "a", "viewer", "user", "ua", "")), (OP_TOUCH, ("namespace", "b", "viewer", "user", "ub", ""))]
        e.write(ups)
        o.write(ups)
        loop = client.run_watch_set(e, ws, sinks, polls=1)
        first = next(loop)
        assert code_of(aclgpu, lambda: next(client.run_watch_set(e, ws, sinks, polls=1))) == aclgpu.ERR_FAILED_PRECONDITION  # no second poller
        stream = [first] + list(loop)
        want_a, want_b = o.lookup("pod", "view", "user", "ua"), o.lookup("pod", "view", "user", "ub")
        assert len(want_a) == len(want_b) == 10 and not (want_a & want_b)
        assert {oid for _ok, oid in got[wa]} == want_a and {oid for _ok, oid in got[wb]} == want_b  # neither watcher's changes were eaten
        assert all(ok for ok, _oid in got[wa] + got[wb])
        assert stream == [(ok, oid, wa) for ok, oid in got[wa]] + [(ok, oid, wb) for ok, oid in got[wb]]
        # one loses it again: only that watcher's sink hears of it
        ups = [(OP_DELETE, ("namespace", "b", "viewer", "user", "ub", ""))]
        e.write(ups)
        o.write(ups)
        got[wa].clear()
        got[wb].clear()
        assert len(list(client.run_watch_set(e, ws, sinks, polls=1))) == 10
        assert got[wa] == [] and {oid for ok, oid in got[wb] if not ok} == want_b and o.lookup("pod", "view", "user", "ub") == set()

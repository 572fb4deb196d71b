"""Check on SLOW hashed rows (plan.hpp: two-choice rows, and single-choice rows of 2^16 buckets and more), equal to the oracle item by item.
The kernels gather every hashed-row probe at hrow_fast and redo the slow lanes of a wave behind a ballot (kernels.hip simple_steps and
flush_probes' probe; bucket_row_contains in the generic interpreter): none of the suite's other graphs holds a row of 2^16 buckets.  The
graph (tests/hashed_rows_graph.py; its shapes are asserted by tests/test_hashed_rows_cpu.py) puts big users with rows of every shape next to
ordinary users with fast rows in the same waves, at ragged batch sizes, through the walk, the level loop, the walk overflowing into the
loop, the device-resident entry point and logical shards; then the depth limit behind a slow row, a slow `user:*` row under `&` / `-`,
the reverse routes, the write path, and every row two-choice in a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import orc
from tests import hashed_rows_graph as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
NT = 16
RAGGED = (1, 63, 65, 4097, 100_000)


@pytest.fixture(scope="module")
def aclgpu(aclgpu_lib):
    import aclgpu as m
    return m


def _pick(sorted_r, sorted_s, keys, r):
    st = np.searchsorted(sorted_r, keys, side="left")
    en = np.searchsorted(sorted_r, keys, side="right")
    ok = en > st
    p = st + (r % np.maximum(en - st, 1))
    return ok, sorted_s[np.minimum(p, sorted_s.size - 1)]


def _edges(E, rt, rel, st, sr=""):
    for e in E:
        if e[:4] == (rt, rel, st, sr):
            o = np.argsort(e[4], kind="stable")
            return e[4][o], e[5][o]
    raise KeyError((rt, rel, st, sr))


CATS = ("direct", "namespace", "depth1", "depth2", "depth3", "depth4", "depth5", "miss")


def _requests(E, n, seed=9):
    """pod#view@user items: big and ordinary subjects interleaved two by two, resources by category (CATS)"""
    rng = np.random.default_rng(seed)
    cat = rng.integers(0, len(CATS), size=n)
    big = (np.arange(n) // 2) % 2 == 0
    sub = np.where(big, (np.arange(n) // 4) % H.N_BIG, rng.integers(H.N_BIG, H.N_USER, size=n)).astype(np.uint32)
    res = rng.integers(0, H.N_POD, size=n).astype(np.uint32)
    R = lambda: rng.integers(0, 1 << 30, size=n)  # noqa: E731
    pv_r, pv_s = _edges(E, "pod", "viewer", "user")
    order = np.argsort(pv_s, kind="stable")
    ok, p = _pick(pv_s[order], pv_r[order], sub, R())  # a pod the subject views directly
    m = (cat == 0) & ok
    res[m] = p[m]
    pod_r, pod_ns = _edges(E, "pod", "namespace", "namespace")
    nv_r, nv_s = _edges(E, "namespace", "viewer", "user")
    order = np.argsort(nv_s, kind="stable")
    ok, ns = _pick(nv_s[order], nv_r[order], sub, R())  # a namespace the subject views -> one of its pods
    o2 = np.argsort(pod_ns, kind="stable")
    ok2, p = _pick(pod_ns[o2], pod_r[o2], ns, R())
    m = (cat == 1) & ok & ok2
    res[m] = p[m]
    pg_r, pg_s = _edges(E, "pod", "viewer", "group", "member")
    gg_r, gg_s = _edges(E, "group", "member", "group", "member")
    gu_r, gu_s = _edges(E, "group", "member", "user")
    for k in range(1, 6):  # a pod viewed by a top-level group, k - 1 levels down, a user member of that group (for ordinary subjects)
        idx = np.flatnonzero(cat == k + 1)
        e = rng.integers(0, pg_r.size, size=idx.size)
        pod, g = pg_r[e], pg_s[e].copy()
        alive = np.ones(idx.size, dtype=bool)
        for _ in range(k - 1):
            ok, child = _pick(gg_r, gg_s, g, rng.integers(0, 1 << 30, size=idx.size))
            alive &= ok
            g = np.where(ok, child, g)
        ok, u = _pick(gu_r, gu_s, g, rng.integers(0, 1 << 30, size=idx.size))
        res[idx] = np.where(alive, pod, res[idx])
        ordi = ~big[idx] & ok & alive
        sub[idx[ordi]] = u[ordi]
    return res, sub, cat


@pytest.fixture(scope="module")
def graph():
    E, n = H.big_graph()
    o = orc.Oracle(H.SCHEMA)
    H.load(o, E)
    o.freeze()
    res, sub, cat = _requests(E, max(RAGGED))
    op, oe = o.check_bulk_ids_mt(NT, "pod", "view", res, "user", "", sub)
    for c, name in enumerate(CATS):  # every category answers somewhere, and misses occur
        assert (op[cat == c] == orc.PERM_HAS).any(), name
    assert (op == orc.PERM_NO).sum() > 1000
    for s in H.BIG:  # hits and misses on the same slow rows
        sel = sub == s
        assert (op[sel] == orc.PERM_HAS).any() and (op[sel] == orc.PERM_NO).any(), s
    chain = (H.CHAIN_BASE + np.arange(H.DEPTH_CHAIN - 1)).astype(np.uint32)
    cp, ce = o.check_bulk_ids("group", "member", chain, "user", "", np.zeros(chain.size, dtype=np.uint32))
    assert (cp == orc.PERM_HAS).any() and (ce == orc.ERR_DEPTH).any()  # within the limit and beyond it
    return dict(E=E, n=n, o=o, res=res, sub=sub, op=op, oe=oe, chain=chain, cp=cp, ce=ce)


def _ragged(run, g):
    """run(res, sub) -> (perm, err) at every RAGGED size, from different offsets of the request arrays"""
    off = 0
    for sz in RAGGED:
        lo = off % (g["res"].size - sz + 1)
        p, er = run(g["res"][lo:lo + sz], g["sub"][lo:lo + sz])
        want_p, want_e = g["op"][lo:lo + sz], g["oe"][lo:lo + sz]
        assert np.array_equal(p, want_p) and np.array_equal(er, want_e), (sz, int((p != want_p).sum()), int((er != want_e).sum()))
        off += 7919 * sz


@pytest.mark.parametrize("mode", ["walk", "level-loop", "overflow", "device"])
def test_slow_rows_check_parity(mode, graph, aclgpu, monkeypatch):
    g = graph
    if mode == "level-loop":
        monkeypatch.setenv("ACL_LOCAL_MAX", "0")  # (read at acl_open)
    if mode == "overflow":
        monkeypatch.setenv("ACL_LOCAL_CAP", "256")
    with aclgpu.Engine(H.SCHEMA, device=0) as e:
        H.load(e, g["E"])
        if mode == "device":
            import torch

            def run(res, sub):
                items = e.make_items("pod", "view", res, "user", "", sub)
                d_items = torch.from_numpy(items.view(np.uint8).copy()).cuda()
                d_perm = torch.zeros(items.size, dtype=torch.uint8, device="cuda")
                d_err = torch.zeros(items.size, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                e.check_bulk_ids_device(d_items.data_ptr(), items.size, d_perm.data_ptr(), d_err.data_ptr())
                e.sync()
                return d_perm.cpu().numpy(), d_err.cpu().numpy()
        else:
            def run(res, sub):
                return e.check_bulk_ids(e.make_items("pod", "view", res, "user", "", sub))
        e.stats_reset()
        _ragged(run, g)
        st = e.stats()
        if mode in ("walk", "device"):
            assert st["local_passes"] >= len(RAGGED) and st["expand_launches"] == 0, st
        elif mode == "level-loop":
            assert st["local_passes"] == 0 and st["expand_launches"] > 0, st
        else:
            assert st["expand_launches"] > 0, st
        # the depth limit behind a slow row: a group#member chain of 59 groups whose last member group holds user 0 in its 65 536-bucket row
        if mode != "device":
            p, er = e.check_bulk_ids(e.make_items("group", "member", g["chain"], "user", "", np.zeros(g["chain"].size, dtype=np.uint32)))
            assert np.array_equal(p, g["cp"]) and np.array_equal(er, g["ce"])
        if mode == "walk":
            # LookupResources and the keep call (the reverse rows and the bulk Check) for big subjects
            o = g["o"]
            for s in (4, 7):
                got = e.lookup_ids("pod", "view", "user", "", s)
                assert np.array_equal(got, np.sort(o.lookup_ids("pod", "view", "user", "", s))), s
            rng = np.random.default_rng(5)
            for s in (0, 6):
                res = rng.integers(0, H.N_POD, size=5 * 2000).astype(np.uint32)
                sub = np.full(res.size, s, dtype=np.uint32)
                keep = e.check_bulk_keep_ids(e.make_items("pod", "view", res, "user", "", sub), np.arange(0, res.size + 1, 5))
                op, _ = o.check_bulk_ids("pod", "view", res, "user", "", sub)
                want = (op.reshape(-1, 5) == orc.PERM_HAS).all(axis=1)
                assert np.array_equal(keep.astype(bool), want) and want.any() and not want.all(), s


@pytest.mark.parametrize("world", [2, 5])
def test_slow_rows_logical_shards(world, graph, aclgpu):
    from aclgpu import sharded
    g = graph
    engines = []
    lo, n = 1234, 30_000
    res, sub = g["res"][lo:lo + n], g["sub"][lo:lo + n]

    def make(rank, nshards):
        e = aclgpu.Engine(H.SCHEMA, contexts=1)
        H.load(e, g["E"])
        engines.append(e)
        return sharded.GpuShard(e, rank, nshards)

    def run(se):
        items = se.shard.e.make_items("pod", "view", res, "user", "", sub)
        p, er, _stats = se.check_bulk_ids_native(items)
        p2, er2, _ = se.check_bulk_ids_native(items[:65])
        return p.cpu().numpy(), er.cpu().numpy(), p2.cpu().numpy(), er2.cpu().numpy()

    try:
        outs = sharded.run_logical_shards(world, make, run)
    finally:
        for e in engines:
            e.close()
    for p, er, p2, er2 in outs:
        assert np.array_equal(p, g["op"][lo:lo + n]) and np.array_equal(er, g["oe"][lo:lo + n])
        assert np.array_equal(p2, g["op"][lo:lo + 65]) and np.array_equal(er2, g["oe"][lo:lo + 65])


@pytest.mark.parametrize("mode", ["walk", "level-loop"])
def test_slow_wildcard_row_under_combine(mode, aclgpu, monkeypatch):
    """SCHEMA_BANS with a `user:*` row of 65 536 buckets and a user's row of 65 537 (generic interpreter, combine instantiations)."""
    from tests.test_combine_gpu import SCHEMA_BANS
    E, n = H.bans_big_graph()
    o = orc.Oracle(SCHEMA_BANS)
    H.load(o, E)
    o.freeze()
    if mode == "level-loop":
        monkeypatch.setenv("ACL_LOCAL_MAX", "0")
    rng = np.random.default_rng(4)
    B = 60_000
    res = rng.integers(0, n["pod"], size=B).astype(np.uint32)
    sub = np.where(np.arange(B) % 3 == 0, np.arange(B) % 2, rng.integers(0, n["user"], size=B)).astype(np.uint32)
    with aclgpu.Engine(SCHEMA_BANS, device=0) as e:
        H.load(e, E)
        for perm in ("view", "strict", "loose"):
            p, er = e.check_bulk_ids(e.make_items("pod", perm, res, "user", "", sub))
            op, oe = o.check_bulk_ids_mt(NT, "pod", perm, res, "user", "", sub)
            assert np.array_equal(p, op) and np.array_equal(er, oe), (perm, int((p != op).sum()))
            assert 0 < int((op == orc.PERM_HAS).sum()) < B
        st = e.stats()
        if mode == "walk":
            assert st["local_passes"] >= 3 and st["expand_launches"] == 0, st
        else:
            assert st["local_passes"] == 0 and st["expand_launches"] > 0, st


def test_slow_rows_write_path(aclgpu, monkeypatch):
    """tests/test_hashed_rows_cpu.py's write sequence (a fast row turns two-choice in place, another moves past 2^16 buckets, a two-choice row
    is deleted down to empty, an id leaves a seeded slow row and comes back) on a GPU engine: every answer after every step equals the oracle's,
    and every step was an in-place patch of the device snapshot.  (The moved rows leave garbage behind that would soon start a background
    compaction -- a new snapshot swapped in, which is not what this test reads: the slack keeps it off.)"""
    monkeypatch.setenv("ACL_COMPACTION_SLACK", str(1 << 30))  # (read at acl_open)
    E, info = H.write_graph()
    o = orc.Oracle(H.SCHEMA)
    H.intern_write_names(o)
    H.load(o, E)
    rng = np.random.default_rng(6)
    written = np.unique([int(r[1][1:]) for _label, ups in H.write_steps(info) for _op, r in ups])
    groups = np.concatenate([H.W_GROUPS + np.arange(H.W_PARENTS), rng.integers(0, H.W_GROUPS, size=3000), written]).astype(np.uint32)
    res = np.tile(groups, 5)
    sub = np.repeat(np.arange(5), groups.size).astype(np.uint32)
    with aclgpu.Engine(H.SCHEMA, device=0) as e:
        H.intern_write_names(e)
        H.load(e, E)

        def compare(label):
            p, er = e.check_bulk_ids(e.make_items("group", "member", res, "user", "", sub))
            op, oe = o.check_bulk_ids_mt(NT, "group", "member", res, "user", "", sub)
            assert np.array_equal(p, op) and np.array_equal(er, oe), (label, int((p != op).sum()), int((er != oe).sum()))
            return op

        op = compare("initial")
        assert (op == orc.PERM_HAS).any() and (op == orc.PERM_NO).any()
        st0 = e.stats()
        for k, (label, ups) in enumerate(H.write_steps(info), 1):  # (every step patches the snapshot at least once: at its read)
            H.apply_step(e, ups, aclgpu.OP_TOUCH, aclgpu.OP_DELETE)
            H.apply_step(o, ups, orc.OP_TOUCH, orc.OP_DELETE)
            compare(label)
            st = e.stats()
            assert st["snapshot_builds"] == st0["snapshot_builds"] and st["snapshot_compactions"] == st0["snapshot_compactions"], (label, st)
            assert st["snapshot_patches"] >= st0["snapshot_patches"] + k, (label, st["snapshot_patches"], st0["snapshot_patches"])


def test_every_row_two_choice_child(aclgpu_lib):
    """ACL_SEEDED_ROWS=0 (latched per process): the reduced C2 / C4 parity, the bans graph in the walk and the level loop and a short fuzz per
    schema, in a child process where every row is two-choice."""
    env = dict(os.environ, ACL_SEEDED_ROWS="0")
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rows_worker.py")], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    except subprocess.TimeoutExpired as x:
        pytest.fail(f"the two-choice child timed out; its stderr:\n{(x.stderr or b'')[-4000:]}")
    assert p.returncode == 0, f"the two-choice child exited {p.returncode}; its stderr:\n{p.stderr[-4000:]}"
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["seeded_rows"] == "0" and len(out["done"]) == 6, out
    assert out["reports"] and all(r["two"] == r["rows"] > 0 for r in out["reports"]), out["reports"]

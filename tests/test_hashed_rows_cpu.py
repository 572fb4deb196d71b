"""Hashed-row shapes (plan.hpp: fast, slow single-choice, two-choice), read back from the ACL_DEBUG_ROWS report of store-only engines:
the GPU test's graph (tests/test_hashed_rows_gpu.py) holds every shape it is meant to exercise, and writes change a row's shape in place
or move it while the patched snapshot stays exact (acl_selfcheck_snapshot verifies it against the store)."""
import numpy as np
import pytest

from tests import hashed_rows_graph as H


@pytest.fixture(scope="module")
def aclgpu(aclgpu_lib):
    import aclgpu as m
    return m


def _build(aclgpu, E, capfd, schema=H.SCHEMA):
    e = aclgpu.Engine(schema, store_only=True)
    H.load(e, E)
    capfd.readouterr()
    assert e.selfcheck_snapshot_code() == 0
    reps = H.parse_reports(capfd.readouterr().err)
    assert len(reps) == 1, reps
    return e, reps[0]


def test_report_lists_every_slow_row(aclgpu, capfd, monkeypatch):
    monkeypatch.setenv("ACL_DEBUG_ROWS", "2")
    rows = [np.arange(10), np.arange(1_000, 1_000 + H.CONSEC_65536), np.random.default_rng(1).choice(50_000, 1_500, replace=False)]
    E = [("group", "member", "user", "", np.concatenate(rows).astype(np.uint32), np.repeat(np.arange(3), [r.size for r in rows]).astype(np.uint32))]
    e, rep = _build(aclgpu, E, capfd)
    assert rep["rows"] == 3 and rep["ids"] == sum(r.size for r in rows) and rep["slow"] == len(rep["slow_rows"]) == 2
    assert rep["slow_rows"][("group#member@user", 1)] == dict(nb=65536, two=0, seed=rep["slow_rows"][("group#member@user", 1)]["seed"], ids=H.CONSEC_65536)
    assert rep["slow_rows"][("group#member@user", 2)]["two"] == 1 and rep["slow_rows"][("group#member@user", 2)]["ids"] == 1_500
    assert rep["largest"] == 65536 and 0 < rep["largest_fast"] < 16
    monkeypatch.setenv("ACL_DEBUG_ROWS", "1")  # the summary alone
    e2, rep2 = _build(aclgpu, E, capfd)
    assert rep2["slow"] == 2 and rep2["slow_rows"] == {}
    for x in (e, e2):
        x.close()


def test_gpu_graph_has_every_shape(aclgpu, capfd, monkeypatch):
    monkeypatch.setenv("ACL_DEBUG_ROWS", "2")
    E, _ = H.big_graph()
    e, rep = _build(aclgpu, E, capfd)
    for sid, want in H.BIG.items():
        for rel, shape in want:
            assert H.shape_of(rep, rel, sid) == shape, (sid, rel, rep["slow_rows"].get((rel, sid)))
    seen = {H.shape_of(rep, rel, sid) for sid, want in H.BIG.items() for rel, _ in want}
    assert {"fast", "two<", "two>=", "nb=65536", "nb=65537"} <= seen
    # 65 536 and 65 537 buckets: the 16-bit bucket count the fast hash sees is 0 and 1
    assert {r["nb"] & 0xFFFF for r in rep["slow_rows"].values() if not r["two"]} >= {0, 1}
    # the big users are the only slow rows; every other row (ordinary users, 8 groups each) is fast
    assert {sid for (_rel, sid) in rep["slow_rows"]} <= set(H.BIG)
    assert rep["rows"] > 10_000 and rep["largest_fast"] == 65535 and rep["largest"] >= 1 << 16
    e.close()


def test_largest_fast_row_is_pinned(aclgpu, capfd, monkeypatch):
    """FAST_MAX_CONSEC consecutive ids: the builder's fast row of 65 535 buckets; one id more: a seeded slow row of 65 536 (searched here, then
    pinned).  A full row (3 ids in every bucket under seed 0) is fast at 65 535 buckets too, at load 0.75."""
    monkeypatch.setenv("ACL_DEBUG_ROWS", "2")
    for n, fast, nb in ((H.FAST_MAX_CONSEC, True, 65535), (H.FAST_MAX_CONSEC + 1, False, 65536)):
        E = [("group", "member", "user", "", np.arange(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32))]
        e, rep = _build(aclgpu, E, capfd)
        assert rep["rows"] == 1 and rep["ids"] == n
        assert (rep["largest_fast"], rep["slow"]) == ((nb, 0) if fast else (0, 1)), rep
        assert rep["largest"] == nb
        e.close()
    full, _ = H.full_fast_row(65535)
    E = [("group", "member", "user", "", full.astype(np.uint32), np.zeros(full.size, dtype=np.uint32))]
    e, rep = _build(aclgpu, E, capfd)
    assert full.size == 3 * 65535 and (rep["largest_fast"], rep["slow"], rep["ids"]) == (65535, 0, full.size)
    e.close()


def test_shape_changes_under_writes(aclgpu, capfd, monkeypatch):
    monkeypatch.setenv("ACL_DEBUG_ROWS", "2")
    e = aclgpu.Engine(H.SCHEMA, store_only=True)
    H.intern_write_names(e)
    E, info = H.write_graph()
    H.load(e, E)
    capfd.readouterr()
    assert e.selfcheck_snapshot_code() == 0
    rep = H.parse_reports(capfd.readouterr().err)[-1]
    rel = "group#member@user"
    shape = lambda r, sid: H.shape_of(r, rel, sid)  # noqa: E731
    assert [shape(rep, k) for k in range(5)] == ["fast", "fast", "two<", "nb=65536", "fast"]
    assert rep["largest_fast"] == 65535
    ids0 = rep["ids"]
    for label, ups in H.write_steps(info):
        assert len(ups) <= 8192
        H.apply_step(e, ups, aclgpu.OP_TOUCH, aclgpu.OP_DELETE)
        assert e.selfcheck_snapshot_code() == 1, label  # patched in place (and verified against the store), not rebuilt
        reps = H.parse_reports(capfd.readouterr().err)
        assert len(reps) == 1, label
        rep = reps[0]
        ids0 += sum(1 if o == "touch" else -1 for o, _ in ups)
        assert rep["ids"] == ids0, label
        row = lambda sid: rep["slow_rows"].get((rel, sid))  # noqa: E731
        if label == "u1-make-room":
            assert shape(rep, 1) == "fast"
        elif label == "u1-collide":  # two-choice in the same 65 535 buckets
            assert row(1) == dict(nb=65535, two=1, seed=0, ids=3 * 65535)
        elif label == "u4-collide":  # moved: seeded slow, 2^16 buckets and more
            assert row(4)["two"] == 0 and row(4)["nb"] >= 1 << 16 and row(4)["ids"] == 3 * 65534 + 2
        elif label == "u2-delete-some":
            assert row(2)["two"] == 1 and row(2)["ids"] == 1_300
        elif label == "u2-delete-rest":
            assert row(2) is None  # empty: nothing left to place two-choice
        elif label == "u3-remove":
            assert row(3)["nb"] == 65536 and row(3)["ids"] == H.CONSEC_65536 - 1
        elif label == "u3-readd":
            assert row(3)["nb"] == 65536 and row(3)["ids"] == H.CONSEC_65536
    assert shape(rep, 0) == "fast"  # untouched
    e.close()


def test_all_rows_two_choice_in_a_fresh_process():
    """ACL_SEEDED_ROWS=0 is latched once per process: a child sees it, and then every row of a graph is two-choice."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ACL_SEEDED_ROWS="0")
    p = subprocess.run([sys.executable, os.path.join(root, "tests", "rows_worker.py"), "--cpu"], env=env, capture_output=True, text=True, timeout=300,
                       cwd=root)
    assert p.returncode == 0, p.stderr[-4000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["reports"] and all(r["two"] == r["rows"] > 0 for r in out["reports"]), out

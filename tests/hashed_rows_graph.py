"""Graphs with hashed rows of every shape (plan.hpp): fast rows, two-choice rows below and above 2^16 buckets, seeded slow rows at
exactly 65 536 and 65 537 buckets and the largest fast row the builder makes.  Shared by tests/test_hashed_rows_cpu.py (which reads
every shape back from the ACL_DEBUG_ROWS report) and tests/test_hashed_rows_gpu.py (which compares Check on them with the oracle).
Test infrastructure, not a test module."""
from __future__ import annotations

import re

import numpy as np

from aclgpu.workloads import SCHEMA_C4

# ---- the ACL_DEBUG_ROWS report (plan.cpp debug_rows_report)
_SUMMARY = re.compile(r"\[aclgpu\] hashed rows: (\d+) \((\d+) two-choice holding (\d+) buckets\), (\d+) ids in (\d+) buckets .*; "
                      r"slow (\d+), largest (\d+) buckets, largest fast (\d+) buckets")
_SLOW = re.compile(r"\[aclgpu\] slow row: (\w+)#(\w+)@(\w+)(:\*)? sid=(\d+) nb=(\d+) two=(\d) seed=(\d+) ids=(\d+)")


def parse_reports(text: str):
    """-> [report]: one per summary line, each {'rows', 'two', 'ids', 'slow', 'largest', 'largest_fast', 'slow_rows': {(rel, sid): row}}
    with row = {'nb', 'two', 'seed', 'ids'}; rel = 'type#relation@subject' (+ ':*' for a wildcard row).  The per-row lines of a report
    come before its summary."""
    out, pending = [], {}
    for line in text.splitlines():
        m = _SLOW.search(line)
        if m:
            rel = f"{m.group(1)}#{m.group(2)}@{m.group(3)}{m.group(4) or ''}"
            pending[(rel, int(m.group(5)))] = dict(nb=int(m.group(6)), two=int(m.group(7)), seed=int(m.group(8)), ids=int(m.group(9)))
            continue
        m = _SUMMARY.search(line)
        if m:
            out.append(dict(rows=int(m.group(1)), two=int(m.group(2)), ids=int(m.group(4)), slow=int(m.group(6)), largest=int(m.group(7)),
                            largest_fast=int(m.group(8)), slow_rows=pending))
            pending = {}
    return out


# ---- the fast hash (plan.hpp hrow_fast) restated, to choose ids that a seed-0 fast row places at load 0.75
def hrow_fast_np(ids: np.ndarray, nb: int, seed: int = 0) -> np.ndarray:
    t = (ids.astype(np.uint64) ^ (ids.astype(np.uint64) >> np.uint64(12)) ^ np.uint64(seed)) & np.uint64(0xFFFFFF)
    h = (t * np.uint64(0x9E3779)) & np.uint64(0xFFFFFFFF)
    return (((h >> np.uint64(8)) & np.uint64(0xFFFF)) * np.uint64(nb & 0xFFFF) >> np.uint64(16)).astype(np.int64)


def full_fast_row(nb: int = 65535, per_bucket: int = 3, space: int = 1 << 20):
    """ids (ascending) that seed 0 spreads exactly `per_bucket` per bucket over `nb` buckets: with per_bucket = 3 the builder makes
    them a FAST row of nb buckets at load 0.75 (n = 3 nb -> buckets_for(n) = nb, seed 0 places them); plus, for one bucket, two more
    ids that hash there -- the fifth id in that bucket breaks seed 0."""
    cand = np.arange(space, dtype=np.uint32)
    b = hrow_fast_np(cand, nb)
    order = np.argsort(b, kind="stable")
    bs = b[order]
    first = np.searchsorted(bs, np.arange(nb))
    cnt = np.searchsorted(bs, np.arange(nb), side="right") - first
    assert cnt.min() >= per_bucket + 2, "id space too small"
    take = (first[:, None] + np.arange(per_bucket)[None, :]).reshape(-1)
    ids = np.sort(cand[order[take]])
    extra = cand[order[first[0] + per_bucket: first[0] + per_bucket + 2]]
    return ids, extra


# ---- the GPU test's graph: SCHEMA_C4, numeric ids
LEVELS, PER_LEVEL = 5, 4000        # nested groups: level l group i has id 5 i + l (ids < 20 000), contains 1-4 groups of level l + 1
N_GROUP, N_NS, N_POD, N_USER = 600_000, 200_000, 200_000, 20_000
CONSEC_65536, CONSEC_65537 = 196_606, 196_609  # consecutive ids: seeded slow rows of exactly 65 536 / 65 537 buckets
FAST_MAX_CONSEC = 109_107  # consecutive ids 0..109106: the builder's fast row of 65 535 buckets (109 108 ids -> 65 536, slow); searched, then pinned
DEPTH_CHAIN = 60           # group#member chain longer than the 50-dispatch limit
CHAIN_BASE = 500_000

# big subjects (user ids) and the row each is meant to have: (relation, expected shape); shapes: 'fast', 'two<', 'two>=', 'nb=65536', 'nb=65537'
BIG = {
    0: [("group#member@user", "nb=65536")],   # groups [10 000, 206 606): half of every nesting level, the chain's last group
    1: [("group#member@user", "nb=65537")],   # groups [10 001, 206 610)
    2: [("group#member@user", "fast")],       # 196 605 ids that seed 0 fills 3 per bucket: a fast row of 65 535 buckets at load 0.75
    3: [("group#member@user", "two>=")],      # 200 000 random groups of 600 000
    4: [("group#member@user", "two<")],       # 2 000 random nesting-level groups
    5: [("group#member@user", "fast")],       # FAST_MAX_CONSEC consecutive groups from 0
    6: [("namespace#viewer@user", "nb=65536"), ("namespace#creator@user", "fast")],  # flush_probes: first probe slow, second fast
    7: [("namespace#viewer@user", "fast"), ("namespace#creator@user", "two<")],      # ... first fast, second slow
    8: [("pod#viewer@user", "nb=71191"), ("pod#creator@user", "nb=65537")],          # a CI bot: 196 609 pods created; views 150 000 random pods
}
N_BIG = 9


def big_graph(seed: int = 0x5EED):
    """-> (edges [(rtype, rel, stype, srel, res, subj)], nobjects)"""
    rng = np.random.default_rng(seed)
    E = []
    u32 = lambda a: np.ascontiguousarray(a, dtype=np.uint32)  # noqa: E731
    ordinary = lambda n: rng.integers(N_BIG, N_USER, size=n).astype(np.uint32)  # noqa: E731
    # nesting: level l -> level l + 1
    par, kid = [], []
    for lv in range(LEVELS - 1):
        i = np.repeat(np.arange(PER_LEVEL), 4)
        j = rng.integers(0, PER_LEVEL, size=i.size)
        par.append(5 * i + lv)
        kid.append(5 * j + lv + 1)
    gr, gs = np.unique(np.stack([np.concatenate(par), np.concatenate(kid)]), axis=1)
    chain = CHAIN_BASE + np.arange(DEPTH_CHAIN - 1)   # chain[k] contains chain[k + 1]; the last one contains group 206 605 (in user 0's row)
    gr = np.concatenate([gr, chain])
    gs = np.concatenate([gs, np.append(chain[1:], 206_605)])
    E.append(("group", "member", "group", "member", u32(gr), u32(gs)))
    # user members: ordinary users, ~8 per nesting-level group; then the big users' rows
    lvl = np.arange(LEVELS * PER_LEVEL)
    r, s = np.repeat(lvl, 8), ordinary(8 * lvl.size)
    rows = [(r, s)]
    rows.append((np.arange(10_000, 10_000 + CONSEC_65536), 0))
    rows.append((np.arange(10_001, 10_001 + CONSEC_65537), 1))
    rows.append((full_fast_row()[0], 2))
    rows.append((rng.choice(N_GROUP, 200_000, replace=False), 3))
    rows.append((rng.choice(LEVELS * PER_LEVEL, 2_000, replace=False), 4))
    rows.append((np.arange(FAST_MAX_CONSEC), 5))
    res = np.concatenate([x[0] for x in rows])
    sub = np.concatenate([x[1] if isinstance(x[1], np.ndarray) else np.full(x[0].size, x[1]) for x in rows])
    key = np.unique(res.astype(np.uint64) << np.uint64(32) | sub.astype(np.uint64))
    E.append(("group", "member", "user", "", u32(key >> np.uint64(32)), u32(key & np.uint64(0xFFFFFFFF))))
    # namespaces
    nss = np.arange(N_NS)
    vr = np.concatenate([nss, np.arange(CONSEC_65536), rng.choice(N_NS, 40, replace=False)])
    vs = np.concatenate([ordinary(N_NS), np.full(CONSEC_65536, 6), np.full(40, 7)])
    key = np.unique(vr.astype(np.uint64) << np.uint64(32) | vs.astype(np.uint64))
    E.append(("namespace", "viewer", "user", "", u32(key >> np.uint64(32)), u32(key & np.uint64(0xFFFFFFFF))))
    ng = rng.choice(N_NS, 20_000, replace=False)
    E.append(("namespace", "viewer", "group", "member", u32(ng), u32(5 * rng.integers(0, PER_LEVEL, size=ng.size))))
    cr = np.concatenate([nss, rng.choice(N_NS, 30, replace=False), rng.choice(N_NS, 3_000, replace=False)])
    cs = np.concatenate([ordinary(N_NS), np.full(30, 6), np.full(3_000, 7)])
    key = np.unique(cr.astype(np.uint64) << np.uint64(32) | cs.astype(np.uint64))
    E.append(("namespace", "creator", "user", "", u32(key >> np.uint64(32)), u32(key & np.uint64(0xFFFFFFFF))))
    # pods
    pods = np.arange(N_POD)
    E.append(("pod", "namespace", "namespace", "", u32(pods), u32(rng.integers(0, N_NS, size=N_POD))))
    pg = rng.choice(N_POD, 100_000, replace=False)
    E.append(("pod", "viewer", "group", "member", u32(pg), u32(5 * rng.integers(0, PER_LEVEL, size=pg.size))))
    pr = np.concatenate([rng.integers(0, N_POD, size=N_POD // 2), np.sort(rng.choice(N_POD, 150_000, replace=False))])
    ps = np.concatenate([ordinary(N_POD // 2), np.full(150_000, 8)])
    key = np.unique(pr.astype(np.uint64) << np.uint64(32) | ps.astype(np.uint64))
    E.append(("pod", "viewer", "user", "", u32(key >> np.uint64(32)), u32(key & np.uint64(0xFFFFFFFF))))
    cr = np.concatenate([np.arange(CONSEC_65537, N_POD), np.arange(CONSEC_65537)])
    cs = np.concatenate([ordinary(N_POD - CONSEC_65537), np.full(CONSEC_65537, 8)])
    E.append(("pod", "creator", "user", "", u32(cr), u32(cs)))
    return E, dict(user=N_USER, group=N_GROUP, namespace=N_NS, pod=N_POD)


def load(target, E):
    for rt, rel, st, sr, res, subj in E:
        target.add_edges(rt, rel, st, sr, res, subj)


def shape_of(report, rel: str, sid: int) -> str:
    """'fast' (no slow-row line), 'two<' / 'two>=' (two-choice below / at or above 2^16 buckets), or 'nb=<buckets>' (seeded slow)"""
    r = report["slow_rows"].get((rel, sid))
    if r is None:
        return "fast"
    if r["two"]:
        return "two<" if r["nb"] < 1 << 16 else "two>="
    return f"nb={r['nb']}"


# ---- wildcard + combine: SCHEMA_BANS (tests/test_combine_gpu.py) with a slow `user:*` row and a slow user row
def bans_big_graph():
    from tests.test_combine_gpu import bans_graph
    E, n = bans_graph(11, n_pod=200_000)
    E = list(E)
    E.append(("pod", "viewer", "user", "*", np.arange(CONSEC_65536, dtype=np.uint32), np.zeros(CONSEC_65536, dtype=np.uint32)))
    E.append(("pod", "viewer", "user", "", np.arange(3, 3 + CONSEC_65537, dtype=np.uint32), np.full(CONSEC_65537, 1, dtype=np.uint32)))
    return E, n


SCHEMA = SCHEMA_C4


# ---- shape changes under writes (named objects: group "g<i>" has id i, user "u<k>" id k -- interned in that order before the bulk load)
W_GROUPS, W_PARENTS, W_KIDS = 210_000, 200, 50   # groups g0..g209999; then parent groups g210000.. containing W_KIDS groups each (simple_steps)


def write_graph(seed: int = 0xC0DE):
    """-> (edges, info).  u0: FAST_MAX_CONSEC consecutive groups (fast, 65 535 buckets); u1: a full fast row of 65 535 buckets (load 0.75);
    u2: 1 500 random groups (two-choice); u3: CONSEC_65536 consecutive groups (seeded slow, 65 536 buckets); u4: a full fast row of
    65 534 buckets."""
    rng = np.random.default_rng(seed)
    full1, extra1 = full_fast_row(65535)
    full4, extra4 = full_fast_row(65534)
    assert max(full1.max(), full4.max(), extra1.max(), extra4.max()) < W_GROUPS
    rows = [np.arange(FAST_MAX_CONSEC), full1, np.sort(rng.choice(W_GROUPS, 1_500, replace=False)), np.arange(5_000, 5_000 + CONSEC_65536), full4]
    res = np.concatenate(rows)
    sub = np.concatenate([np.full(r.size, k) for k, r in enumerate(rows)])
    par = W_GROUPS + np.repeat(np.arange(W_PARENTS), W_KIDS)
    kid = rng.integers(0, W_GROUPS, size=par.size)
    E = [("group", "member", "user", "", res.astype(np.uint32), sub.astype(np.uint32)),
         ("group", "member", "group", "member", par.astype(np.uint32), kid.astype(np.uint32))]
    return E, dict(rows=rows, extra1=extra1, extra4=extra4)


def intern_write_names(target, n_users: int = 8):
    """the names of write_graph's ids, interned in id order (target: aclgpu.Engine or oracle.orc.Oracle, nothing loaded yet)"""
    for k in range(n_users):
        assert target.intern("user", f"u{k}") == k
    for i in range(W_GROUPS + W_PARENTS):
        assert target.intern("group", f"g{i}") == i


def member(gid, uid):
    return ("group", f"g{int(gid)}", "member", "user", f"u{int(uid)}", "")


def write_steps(info):
    """[(label, [(op, relationship)])]: every write holds at most 8 192 changes (a patch, not a rebuild).  op: 'touch' / 'delete'.
    With write_graph's rows, after
      u1-make-room   u1 still fast (65 535 buckets, 196 603 ids)
      u1-collide     u1 two-choice IN PLACE (65 535 buckets): two ids that seed 0 puts in one full bucket, and no other seed places the row
      u4-collide     u4 moved to 2^16 buckets and more (seeded slow): its 65 534 buckets cannot hold 196 604 ids at load 0.75
      u2-delete-*    u2's two-choice row shrinks (still two-choice), then is empty
      u3-remove / u3-readd   the same id leaves u3's seeded slow row and comes back (65 536 buckets throughout)"""
    rows = info["rows"]
    e1, e4 = info["extra1"], info["extra4"]
    room = [g for g in rows[1] if g not in set(e1.tolist())][-2:]
    r2 = rows[2]
    return [("u1-make-room", [("delete", member(g, 1)) for g in room]),
            ("u1-collide", [("touch", member(e1[0], 1)), ("touch", member(e1[1], 1))]),
            ("u4-collide", [("touch", member(e4[0], 4)), ("touch", member(e4[1], 4))]),
            ("u2-delete-some", [("delete", member(g, 2)) for g in r2[:200]]),
            ("u2-delete-rest", [("delete", member(g, 2)) for g in r2[200:]]),
            ("u3-remove", [("delete", member(77_777, 3))]),
            ("u3-readd", [("touch", member(77_777, 3))])]


def apply_step(target, ups, op_touch, op_delete):
    """one step of write_steps on target (aclgpu.Engine or oracle.orc.Oracle): writes of at most 1 000 updates (the API's limit), read once after"""
    ops = {"touch": op_touch, "delete": op_delete}
    for i in range(0, len(ups), 1000):
        target.write([(ops[o], r) for o, r in ups[i:i + 1000]])

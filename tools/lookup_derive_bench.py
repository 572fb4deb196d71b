"""Principal lookups on C4 (1 M objects, 100 000 users, 5-level nested groups at scale 1.0): "the pods this principal may see, the first 500" for a principal
that is a dense user plus 1 / 8 / 32 groups, by Engine.principal_cursor (one mixed open, one derive on the device, one page; no row crosses PCIe) against
what a caller does without it -- acl_lookup_resources_batch per subject form into pinned rows, a numpy OR, a flatnonzero for the first 500.

  timed:    p50 / p99 of both, alternating on ONE engine in ONE run; every call ends in a device synchronisation inside the library.  derive_ms (HIP events
            around the two launches) from a few extra calls with timing on.  Also: one call for 64 principals of a user + 8 groups each (first page of every
            row), and count_rows for the 64 x 64 overlap matrix of those rows against numpy on host rows.
  checked:  every compared row bit for bit: the derived row's whole id list against the host OR's.

  python tools/lookup_derive_bench.py --out profiles/lookup_derive_c4.json --md profiles/lookup_derive_c4.md        (on a box with the GPU)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "spicedb-kubeapi-proxy_amd"))

GROUPS = (1, 8, 32)
PAGE = 500


def pct(xs, q):
    return round(float(np.percentile(np.asarray(xs) * 1e6, q)), 1)


def ids_of(row):
    return np.flatnonzero(np.unpackbits(np.ascontiguousarray(row).view(np.uint8), bitorder="little")).astype(np.uint32)


def first_ids(row, limit):
    """the first `limit` set bits of a host row: a flatnonzero over growing slices (tools/lookup_page_bench.py page_of_row from the start)"""
    w0, step, got, have = 0, 256, [], 0
    while w0 < row.size and have < limit:
        ids = np.flatnonzero(np.unpackbits(row[w0:w0 + step].view(np.uint8), bitorder="little")) + (w0 << 5)
        got.append(ids)
        have += ids.size
        w0 += step
        step *= 4
    return (np.concatenate(got)[:limit] if got else np.zeros(0, dtype=np.int64)).astype(np.uint32)


def popcounts(rows):
    return np.bitwise_count(rows).sum(axis=-1, dtype=np.uint64) if hasattr(np, "bitwise_count") else np.unpackbits(rows.view(np.uint8), axis=-1).sum(axis=-1, dtype=np.uint64)


def write_md(rows, meta, path):
    out = ["# Principal lookups on C4: a derived cursor against per-form batch calls and a host OR", "",
           f"`tools/lookup_derive_bench.py` on one MI355X, C4 at scale {meta['scale']} ({meta['objects']} objects, {meta['pods']} pods: a row of",
           f"{meta['row_bytes']} bytes). The dense user holds {meta['dense_ids']} pods. `derived` is `Engine.principal_cursor` (one mixed open: one walk",
           f"per subject form; one derive: two launches) plus the first page of {PAGE} ids per principal and the close; `host OR` is",
           "`acl_lookup_resources_batch` per subject form into pinned rows, a numpy OR per principal and a `flatnonzero` over",
           "growing slices for the first page. The two alternate on one engine in one run; times are per call, host clock around",
           "calls that end in a device synchronisation, both driven from Python.",
           f"Rows compared bit for bit: {meta['rows_compared']}, mismatches: {meta['mismatches']}.", "",
           "| principals | groups per principal | derived p50 us | derived p99 us | host OR p50 us | derived / host OR | derive_ms per call | ids in the rows |",
           "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['principals']} | {r['groups']} | {r['derived_p50_us']} | {r['derived_p99_us']} | {r['host_p50_us']} | {r['vs_host']} | {r['derive_ms']} | {r['ids']} |")
    m = meta["overlap"]
    out += ["", f"Overlap matrix of the {m['n']} principal rows ({m['n']} x {m['n']} counts of `all{{i, j}}`): `count_rows` p50 {m['count_p50_us']} us",
            f"(derive_ms {m['derive_ms']}), numpy on the rows held on the host (AND + popcount, a row against all rows per step) p50",
            f"{m['numpy_p50_us']} us; ratio {m['vs_numpy']}. Counts equal: {m['equal']}.", ""]
    with open(path, "w") as f:
        f.write("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--md", default="")
    a = ap.parse_args()
    import aclgpu
    from aclgpu import workloads

    w = workloads.c4(scale=a.scale, batch=4096)
    rows, compared, mism = [], 0, 0
    with aclgpu.Engine(w.schema, device=0) as e:
        w.load(e)
        rng = np.random.default_rng(11)
        sample = np.unique(rng.integers(0, w.nobjects["user"], size=512).astype(np.uint32))
        _b, c = e.lookup_ids_batch("pod", "view", "user", "", sample)
        by_count = sample[np.argsort(c, kind="stable")]
        dense = int(by_count[-1])
        e_pods = e.object_count("pod")
        words = max(1, (e_pods + 31) // 32)

        def pinned_rows(n):
            coff = (n * words * 4 + 7) // 8 * 8
            buf = e.host_alloc(coff + 8 * n)
            return buf, (buf[:n * words * 4].view(np.uint32).reshape(n, words), buf[coff:coff + 8 * n].view(np.uint64))

        def measure(principals, reps):
            """principals: [(user id, [group ids])] -> one table row"""
            nonlocal compared, mism
            P = len(principals)
            users = np.array([u for u, _g in principals], dtype=np.uint32)
            groups = np.array([g for _u, gs in principals for g in gs], dtype=np.uint32)
            G = len(principals[0][1])
            forms = [[("user", "", int(u))] + [("group", "member", int(g)) for g in gs] for u, gs in principals]
            bu, out_u = pinned_rows(P)
            bg, out_g = pinned_rows(max(groups.size, 1))
            reqs = [(p, None, PAGE) for p in range(P)]

            def derived():
                with e.principal_cursor("pod", "view", forms) as cur:
                    return cur.pages(reqs)

            def host():
                ru = e.lookup_ids_batch("pod", "view", "user", "", users, out=out_u)[0]
                rg = e.lookup_ids_batch("pod", "view", "group", "member", groups, out=out_g)[0] if groups.size else None
                res = []
                for p in range(P):
                    row = ru[p] if not G else np.bitwise_or.reduce(rg[p * G:(p + 1) * G], axis=0) | ru[p]
                    res.append((row, first_ids(row, PAGE)))
                return res

            td, th = [], []
            for _ in range(reps + 2):
                t = time.perf_counter()
                got = derived()
                td.append(time.perf_counter() - t)
                t = time.perf_counter()
                want = host()
                th.append(time.perf_counter() - t)
                for p in range(P):
                    mism += int(not np.array_equal(got[p][0], want[p][1]))
            # every compared row, bit for bit: the whole id list of the derived row against the host OR's
            want = host()
            with e.principal_cursor("pod", "view", forms) as cur:
                counts = cur.info()[1]
                whole = cur.pages([(p, None, int(counts[p]) + 1) for p in range(P)])
                for p in range(P):
                    compared += 1
                    mism += int(not np.array_equal(whole[p][0], ids_of(want[p][0])))
            e.set_timing(True)
            e.stats_reset()
            for _ in range(3):
                derived()
            ms = e.stats()["derive_ms"] / 3
            e.set_timing(False)
            e.host_free(bu)
            e.host_free(bg)
            r = {"principals": P, "groups": G, "derived_p50_us": pct(td[2:], 50), "derived_p99_us": pct(td[2:], 99), "host_p50_us": pct(th[2:], 50), "derive_ms": round(ms, 4),
                 "ids": int(counts.sum()), "reps": reps}
            r["vs_host"] = round(r["derived_p50_us"] / r["host_p50_us"], 3)
            rows.append(r)
            print(json.dumps(r), flush=True)

        for G in GROUPS:
            measure([(dense, rng.integers(0, w.nobjects["group"], size=G).tolist())], a.reps)
        many = [(int(u), rng.integers(0, w.nobjects["group"], size=8).tolist()) for u in by_count[-64:]]
        measure(many, max(3, a.reps // 4))
        # the overlap matrix of the 64 principal rows
        n = len(many)
        forms = [[("user", "", u)] + [("group", "member", g) for g in gs] for u, gs in many]
        exprs = [([], [(0, i), (0, j)], []) for i in range(n) for j in range(n)]
        with e.principal_cursor("pod", "view", forms) as cur:
            packed = e._derive_args([cur], exprs)[1:]
            host_rows = np.zeros((n, words), dtype=np.uint32)
            whole = cur.pages([(p, None, int(k) + 1) for p, k in enumerate(cur.info()[1])])
            for p in range(n):
                ids = whole[p][0]
                np.bitwise_or.at(host_rows[p], ids >> 5, np.uint32(1) << (ids & 31))
            tc, tn = [], []
            for _ in range(a.reps + 2):
                t = time.perf_counter()
                counts = e.count_rows([cur], packed)
                tc.append(time.perf_counter() - t)
                t = time.perf_counter()
                ref = np.stack([popcounts(host_rows[i] & host_rows) for i in range(n)])
                tn.append(time.perf_counter() - t)
            equal = bool(np.array_equal(counts.reshape(n, n), ref))
            mism += int(not equal)
            e.set_timing(True)
            e.stats_reset()
            for _ in range(3):
                e.count_rows([cur], packed)
            ms = e.stats()["derive_ms"] / 3
            e.set_timing(False)
        overlap = {"n": n, "count_p50_us": pct(tc[2:], 50), "numpy_p50_us": pct(tn[2:], 50), "derive_ms": round(ms, 4), "equal": equal}
        overlap["vs_numpy"] = round(overlap["count_p50_us"] / overlap["numpy_p50_us"], 3)
        print(json.dumps(overlap), flush=True)
    meta = {"workload": "C4", "scale": a.scale, "objects": int(sum(w.nobjects.values())), "pods": int(e_pods), "row_bytes": int(words * 4), "dense_ids": int(c.max()),
            "rows_compared": compared, "mismatches": mism, "overlap": overlap}
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps({**meta, "rows": rows}) + "\n")
    if a.md:
        write_md(rows, meta, a.md)
    print(json.dumps(meta))
    return 0 if mism == 0 else 1


if __name__ == "__main__":
    sys.exit(main())

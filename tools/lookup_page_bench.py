"""Paged LookupResources on C4 (1 M objects, 100 000 users, 5-level nested groups at scale 1.0): pages of `pod#view` for a dense user served by a lookup
cursor (acl_lookup_cursor_pages: the row stays on the device, only ids cross PCIe) against what a caller does without one -- acl_lookup_resources_batch
into a pinned row and a numpy flatnonzero slice per page, once HOLDING the host row between pages and once RE-WALKING per page -- and against the floor of
holding: the row's whole sorted id list kept on the host, a binary search per page.

  pages:    100 / 500 / 5 000 ids, at 1 / 64 / 1 024 requests per call; the first request of a call starts at the front of the row, the others behind ids
            drawn from the row with a fixed seed;
  timed:    p50 / p99 of the cursor call and p50 of the two baselines (per CALL: all of its pages), alternating on ONE engine in ONE run, into buffers all
            three reuse; every call ends in a device synchronisation inside the library.  page_ms (HIP events around the two launches) from a few extra
            calls with timing on.  The open (walk + rank index) is timed on its own, against the walk into the pinned row.
  checked:  every page of every timed cursor call against the held-row baseline's ids.

  python tools/lookup_page_bench.py --out profiles/lookup_page_c4.json --md profiles/lookup_page_c4.md        (on a box with the GPU)"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "spicedb-kubeapi-proxy_amd"))

PAGES = (100, 500, 5000)
REQUESTS = (1, 64, 1024)
FROM_START = 0xFFFFFFFF


def pct(xs, q):
    return round(float(np.percentile(np.asarray(xs) * 1e6, q)), 1)


def page_of_row(row, after, limit):
    """what a caller with the row on the host does for one page: the set bits behind `after`, cut at `limit` -- a flatnonzero over a slice of the row, 256 words
    first and four times as many each time the slice did not hold `limit` ids (a dense row ends in the first slice, a sparse one does not pay for the whole row)"""
    start = 0 if after == FROM_START else after + 1
    w0, step, got, have = start >> 5, 256, [], 0
    while w0 < row.size and have < limit:
        ids = np.flatnonzero(np.unpackbits(row[w0:w0 + step].view(np.uint8), bitorder="little")) + (w0 << 5)
        if not got:
            ids = ids[np.searchsorted(ids, start):]
        got.append(ids)
        have += ids.size
        w0 += step
        step *= 4
    return (np.concatenate(got)[:limit] if got else np.zeros(0, dtype=np.int64)).astype(np.uint32)


def page_of_ids(S, after, limit):
    """... and the least a caller can pay who keeps the whole sorted id list of the row on the host between pages"""
    return S[(0 if after == FROM_START else np.searchsorted(S, np.uint32(after), side="right")):][:limit]  # (a key of S's own type: no conversion of S per page)


def write_md(rows, meta, path):
    out = ["# Paged LookupResources on C4: a lookup cursor against a row held (or walked again) on the host", "",
           f"`tools/lookup_page_bench.py` on one MI355X, C4 at scale {meta['scale']} ({meta['objects']} objects, {meta['pods']} pods: a row of",
           f"{meta['row_bytes']} bytes). The dense user holds {meta['dense_ids']} pods. Cursor call and baselines alternate on one engine in one run; times are",
           "per call (all of its pages), host clock around calls that end in a device synchronisation. The baselines page with numpy: `held row` and `re-walk`",
           "take a `flatnonzero` over growing slices of the row behind `after`, `held ids` keeps the row's sorted id list and searches it. Their per-page cost",
           "is a Python caller's; the cursor's call is timed from Python too (one ctypes call per CALL, not per page).",
           f"Pages compared: {meta['pages_compared']}, mismatches: {meta['mismatches']}.", "",
           f"Open (walk + rank index, rows left on the device): p50 {meta['open_p50_us']} us; the walk into a pinned host row: p50 {meta['walk_p50_us']} us.", "",
           "| ids per page | requests per call | cursor p50 us | cursor p99 us | held row p50 us | held ids p50 us | re-walk p50 us | cursor / held row | cursor / re-walk | page_ms per call | ids returned |",
           "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['page']} | {r['requests']} | {r['cursor_p50_us']} | {r['cursor_p99_us']} | {r['held_p50_us']} | {r['heldids_p50_us']} | {r['rewalk_p50_us']} | {r['vs_held']} | "
                   f"{r['vs_rewalk']} | {r['page_ms']} | {r['ids']} |")
    out.append("")
    with open(path, "w") as f:
        f.write("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default="")
    ap.add_argument("--md", default="")
    a = ap.parse_args()
    import aclgpu
    from aclgpu import workloads

    w = workloads.c4(scale=a.scale, batch=4096)
    rows, compared, mism = [], 0, 0
    with aclgpu.Engine(w.schema, device=0) as e:
        w.load(e)
        rng = np.random.default_rng(7)
        sample = np.unique(rng.integers(0, w.nobjects["user"], size=512).astype(np.uint32))
        _b, c = e.lookup_ids_batch("pod", "view", "user", "", sample)
        dense = np.ascontiguousarray(sample[np.argsort(c, kind="stable")[-1:]])
        e_pods = e.object_count("pod")
        words = max(1, (e_pods + 31) // 32)
        coff = (words * 4 + 7) // 8 * 8  # (the count behind the row, 8-byte aligned)
        pinned = e.host_alloc(coff + 8)
        out = (pinned[:words * 4].view(np.uint32).reshape(1, words), pinned[coff:coff + 8].view(np.uint64))

        def walk():
            return e.lookup_ids_batch("pod", "view", "user", "", dense, out=out)[0][0]

        row = walk()
        assert row.ctypes.data == pinned.ctypes.data  # (the walk wrote into the pinned row)
        S = page_of_row(row, FROM_START, 1 << 30)
        # the open, against the walk it contains
        t_open, t_walk = [], []
        for _ in range(a.reps + 2):
            t = time.perf_counter()
            cur = e.lookup_cursor("pod", "view", "user", "", dense)
            t_open.append(time.perf_counter() - t)
            cur.close()
            t = time.perf_counter()
            walk()
            t_walk.append(time.perf_counter() - t)
        cur = e.lookup_cursor("pod", "view", "user", "", dense)
        assert cur.info()[1].tolist() == [S.size]
        for P in PAGES:
            for R in REQUESTS:
                reps = a.reps if R == 1 else max(3, a.reps // (3 if R == 64 else 10))
                reqs = np.zeros((R, 4), dtype=np.uint32)
                reqs[:, 1] = S[rng.integers(0, S.size, size=R)]
                reqs[0, 1] = FROM_START
                reqs[:, 2] = P
                ids, n, more = np.zeros(R * P, dtype=np.uint32), np.zeros(R, dtype=np.uint32), np.zeros(R, dtype=np.uint8)

                def cursor_call():
                    e._check(e._L.acl_lookup_cursor_pages(e._h, cur._c, reqs.ctypes.data, R, ids.ctypes.data, R * P, n.ctypes.data, more.ctypes.data, None))

                tc, th, ti, tw = [], [], [], []
                for _ in range(reps + 2):
                    t = time.perf_counter()
                    cursor_call()
                    tc.append(time.perf_counter() - t)
                    t = time.perf_counter()
                    held = [page_of_row(row, int(reqs[q, 1]), P) for q in range(R)]
                    th.append(time.perf_counter() - t)
                    t = time.perf_counter()
                    byids = [page_of_ids(S, int(reqs[q, 1]), P) for q in range(R)]
                    ti.append(time.perf_counter() - t)
                    mism += sum(int(not np.array_equal(x, y)) for x, y in zip(held, byids))
                    t = time.perf_counter()
                    for q in range(R):
                        page_of_row(walk(), int(reqs[q, 1]), P)
                    tw.append(time.perf_counter() - t)
                    for q in range(R):
                        compared += 1
                        mism += int(not (int(n[q]) == held[q].size and np.array_equal(ids[q * P:q * P + held[q].size], held[q])))
                e.set_timing(True)
                e.stats_reset()
                for _ in range(3):
                    cursor_call()
                ms = e.stats()["page_ms"] / 3
                e.set_timing(False)
                r = {"page": P, "requests": R, "cursor_p50_us": pct(tc[2:], 50), "cursor_p99_us": pct(tc[2:], 99), "held_p50_us": pct(th[2:], 50), "heldids_p50_us": pct(ti[2:], 50),
                     "rewalk_p50_us": pct(tw[2:], 50), "page_ms": round(ms, 4), "ids": int(n.sum()), "reps": reps}
                r["vs_held"] = round(r["cursor_p50_us"] / r["held_p50_us"], 3)
                r["vs_rewalk"] = round(r["cursor_p50_us"] / r["rewalk_p50_us"], 3)
                rows.append(r)
                print(json.dumps(r), flush=True)
        cur.close()
        e.host_free(pinned)
    meta = {"workload": "C4", "scale": a.scale, "objects": int(sum(w.nobjects.values())), "pods": int(e_pods), "row_bytes": int(words * 4), "dense_ids": int(S.size),
            "open_p50_us": pct(t_open[2:], 50), "walk_p50_us": pct(t_walk[2:], 50), "pages_compared": compared, "mismatches": mism}
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps({**meta, "rows": rows}) + "\n")
    if a.md:
        write_md(rows, meta, a.md)
    print(json.dumps(meta))
    return 0 if mism == 0 else 1


if __name__ == "__main__":
    sys.exit(main())

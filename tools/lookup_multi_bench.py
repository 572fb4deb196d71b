"""LookupResources against many targets on C4 (1 M objects, 100 000 users, 5-level nested groups at scale 1.0): acl_lookup_resources_multi -- one
reverse walk per subject, every target's row -- against the per-target sequence of acl_lookup_resources_batch calls it replaces.

  subjects: n = 1 (one dense and one sparse user) and n = 64 (the 64 users of a random sample who see the most pods: power users);
  targets:  T = 1, 2, 4 and every slot of the schema, plus two sets of small rows (groups and namespaces only), so that the table covers the row sizes
            between "a few KB" and "every pod row of the schema";
  timed:    p50 / p99 of the multi call and p50 of the sequence, alternating on ONE engine in ONE run, into buffers both reuse; rev_multi_ms (HIP events)
            from a few extra calls with timing on.  Every row of every timed multi call is compared with the sequence's.
The engine is opened with ACL_REV_MULTI_MIN_T=2 and ACL_REV_MULTI_MAX_WORDS=2^31-1, so the one walk is taken at EVERY size (`multi_passes` says so per
row): the table is what the route constants of engine_lookup_multi.cpp are read from, not a run under them.

  python tools/lookup_multi_bench.py --out profiles/lookup_multi_c4.json --md profiles/lookup_multi_c4.md        (on a box with the GPU)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "spicedb-kubeapi-proxy_amd"))

ALL = [("group", "member"), ("namespace", "viewer"), ("namespace", "creator"), ("namespace", "view"),
       ("pod", "namespace"), ("pod", "viewer"), ("pod", "creator"), ("pod", "view")]
SETS = [("T=1", [("pod", "view")]),
        ("T=2 small", [("group", "member"), ("namespace", "view")]),
        ("T=4 small", [("group", "member"), ("namespace", "viewer"), ("namespace", "creator"), ("namespace", "view")]),
        ("T=2", [("namespace", "view"), ("pod", "view")]),
        ("T=4", [("group", "member"), ("namespace", "view"), ("pod", "viewer"), ("pod", "view")]),
        ("all slots", ALL)]


def pct(xs, q):
    return round(float(np.percentile(np.asarray(xs) * 1e6, q)), 1)


def write_md(rows, meta, path):
    out = ["# One reverse walk for many targets on C4: `acl_lookup_resources_multi` against the per-target sequence", "",
           f"`tools/lookup_multi_bench.py` on one MI355X, C4 at scale {meta['scale']} ({meta['objects']} objects). Multi call and sequence alternate on",
           "one engine in one run; the engine is opened with the route knobs wide open, so the one walk (`k_rev_multi`) runs at every size.",
           f"Rows compared: {meta['rows_compared']}, mismatches: {meta['mismatches']}.", "",
           "| subjects | targets | row words per lookup | multi p50 us | multi p99 us | sequence p50 us | multi / sequence | rev_multi_ms per call | multi passes |",
           "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['subjects']} | {r['targets']} | {r['row_words']} | {r['multi_p50_us']} | {r['multi_p99_us']} | {r['seq_p50_us']} | {r['ratio']} | "
                   f"{r['rev_multi_ms']} | {r['multi_passes']} |")
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
    os.environ["ACL_REV_MULTI_MIN_T"] = "2"  # (read at acl_open)
    os.environ["ACL_REV_MULTI_MAX_WORDS"] = str(2 ** 31 - 1)
    import aclgpu
    from aclgpu import workloads

    w = workloads.c4(scale=a.scale, batch=4096)
    rows, compared, mism = [], 0, 0
    with aclgpu.Engine(w.schema, device=0) as e:
        w.load(e)
        rng = np.random.default_rng(7)
        sample = np.unique(rng.integers(0, w.nobjects["user"], size=512).astype(np.uint32))
        _b, c = e.lookup_ids_batch("pod", "view", "user", "", sample)
        order = np.argsort(c, kind="stable")
        power = np.ascontiguousarray(sample[order[-64:]])
        groups = {"1 dense": power[-1:], "1 sparse": np.ascontiguousarray(sample[order[:1]]), "64 power": power}
        for gname, sids in groups.items():
            reps = a.reps if sids.size == 1 else max(5, a.reps // 3)
            for tname, tg in SETS:
                multi = e.lookup_ids_multi(tg, "user", "", sids)
                seq = [e.lookup_ids_batch(rt, pm, "user", "", sids) for rt, pm in tg]
                tm, tseq = [], []
                e.stats_reset()
                for _ in range(reps + 2):
                    t = time.perf_counter()
                    multi = e.lookup_ids_multi(tg, "user", "", sids, out=multi)
                    tm.append(time.perf_counter() - t)
                    t = time.perf_counter()
                    for j, (rt, pm) in enumerate(tg):
                        seq[j] = e.lookup_ids_batch(rt, pm, "user", "", sids, out=seq[j])
                    tseq.append(time.perf_counter() - t)
                    for j in range(len(tg)):
                        compared += sids.size
                        mism += int(not (np.array_equal(multi[0][j], seq[j][0]) and np.array_equal(multi[1][:, j], seq[j][1])))
                passes = e.stats()["rev_multi_passes"]
                e.set_timing(True)
                e.stats_reset()
                for _ in range(3):
                    e.lookup_ids_multi(tg, "user", "", sids, out=multi)
                ms = e.stats()["rev_multi_ms"] / 3
                e.set_timing(False)
                r = {"subjects": gname, "targets": tname, "n_targets": len(tg), "row_words": int(sum(m.shape[1] for m in multi[0])),
                     "multi_p50_us": pct(tm[2:], 50), "multi_p99_us": pct(tm[2:], 99), "seq_p50_us": pct(tseq[2:], 50), "rev_multi_ms": round(ms, 4),
                     "multi_passes": f"{passes}/{reps + 2}", "ids": int(multi[1].sum())}
                r["ratio"] = round(r["multi_p50_us"] / r["seq_p50_us"], 2)
                rows.append(r)
                print(json.dumps(r), flush=True)
    meta = {"workload": "C4", "scale": a.scale, "objects": int(sum(w.nobjects.values())), "rows_compared": compared, "mismatches": mism}
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps({**meta, "rows": rows}) + "\n")
    if a.md:
        write_md(rows, meta, a.md)
    print(json.dumps(meta))
    return 0 if mism == 0 else 1


if __name__ == "__main__":
    sys.exit(main())

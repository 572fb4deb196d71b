"""Explain on C4 (1 M objects, 100 000 users, 5-level nested groups at scale 1.0): profiles/explain_c4.{json,md}.

For 1, 64 and 4 096 granted items of the workload's Check stream, in ONE process on one snapshot:
  acl_explain_bulk_ids        call p50 / p99 and the time of k_explain_local inside it (acl_set_timing: the call's kernel time minus the kernel time of the same Check called on its own)
  acl_check_bulk_ids          of the same items (what Explain adds is the difference)
  acl_lookup_subjects_batch   of the same items' resources: the same walk without the early exit (it lists every subject instead of finding one)
plus the first call's extra time (it builds and uploads the subject rows, whose visited-bit layout the walk uses) and the witnesses' lengths.  Every timed
Explain answer is compared with Check's, and every witness is checked to chain from its item's resource to its item's subject.  No speed bar: the figures
are recorded.

  python tools/explain_bench.py --out profiles/explain_c4.json --md profiles/explain_c4.md        (on a box with the GPU; --quick: fewer calls)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "spicedb-kubeapi-proxy_amd"))


def pct(xs, q):
    return round(float(np.percentile(np.asarray(xs) * 1e6, q)), 1)


def chains(items, off, hops):
    """witnesses that do NOT chain from the item's resource to the item's subject"""
    bad = 0
    for i in range(items.size):
        h = hops[off[i]:off[i + 1]]
        ok = h.size > 0 and h["rid"][0] == items["resource_id"][i] and h["sid"][-1] == items["subject_id"][i] and h["stype"][-1] == items["subject_type"][i]
        ok = ok and np.array_equal(h["sid"][:-1], h["rid"][1:]) and np.array_equal(h["stype"][:-1], h["rtype"][1:])
        bad += int(not ok)
    return bad


def write_md(res, path):
    out = ["# Explain on C4: call time next to Check and LookupSubjects", "",
           f"`tools/explain_bench.py` on one MI355X, C4 at scale {res['scale']} ({res['relationships']} relationships), granted items of the workload's Check stream.",
           "One process, one snapshot; `explain kernel` is the call's event-timed kernel time (`acl_set_timing`) minus that of the same",
           "Check called on its own, the other columns are host wall-clock times of whole calls.  `LookupSubjects` lists every holder of",
           "the same items' resources: the same walk without the early exit.", "",
           "| items | Explain p50 us | Explain p99 us | explain kernel us (mean) | Check p50 us | LookupSubjects p50 us | hops per witness (mean / max) |", "|---|---|---|---|---|---|---|"]
    for n, c in res["calls"].items():
        out.append(f"| {n} | {c['explain_p50_us']} | {c['explain_p99_us']} | {c['explain_kernel_us']} | {c['check_p50_us']} | {c['lookup_subjects_p50_us']} | "
                   f"{c['hops_mean']} / {c['hops_max']} |")
    out += ["", f"First Explain call on the snapshot: {res['first_call_ms']} ms (it builds and uploads the subject rows: {res['subject_rows_bytes']} bytes).",
            f"Answers compared with Check: {res['answers_compared']}, mismatches: {res['mismatches']}; witnesses that do not chain: {res['broken_chains']}; "
            f"log overflow retries: {res['overflow_retries']}.", ""]
    with open(path, "w") as f:
        f.write("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--quick", action="store_true", help="fewer calls")
    ap.add_argument("--out", default="", help="write the JSON line to this file")
    ap.add_argument("--md", default="", help="write the markdown note to this file")
    a = ap.parse_args()
    import aclgpu
    from aclgpu import workloads

    t0 = time.perf_counter()
    w = workloads.c4(scale=a.scale, batch=16384)
    res = {"workload": "C4", "scale": a.scale, "relationships": w.ntuples, "calls": {}}
    with aclgpu.Engine(w.schema, device=0) as e:
        w.load(e)
        stream = e.make_items("pod", "view", w.res, "user", "", w.subj)
        perm, err = e.check_bulk_ids(stream)  # (builds the forward snapshot)
        items = stream[(perm == aclgpu.PERM_HAS) & (err == 0)][:4096]
        res["load_s"] = round(time.perf_counter() - t0, 2)
        b0 = e.stats()["snapshot_bytes"]
        t = time.perf_counter()
        e.explain_ids(items[:1])
        res["first_call_ms"] = round((time.perf_counter() - t) * 1e3, 2)
        res["subject_rows_bytes"] = int(e.stats()["snapshot_bytes"] - b0)
        r0 = e.stats()["overflow_retries"]
        e.set_timing(True)
        mism = broken = compared = 0
        for n in [k for k in (1, 64, 4096) if k <= items.size]:
            reps = (3 if a.quick else 30) if n < 4096 else (2 if a.quick else 8)
            xs, cs, ls, km, hop_n = [], [], [], [], []
            pods = np.ascontiguousarray(items["resource_id"][:n])
            for k in range(reps + 2):
                it = items[:n] if n > 1 else items[k % items.size:k % items.size + 1]
                s0 = e.stats()
                t = time.perf_counter()
                p, er, fl, off, hops = e.explain_ids(it)
                xs.append(time.perf_counter() - t)
                s1 = e.stats()
                t = time.perf_counter()
                cp, ce = e.check_bulk_ids(it)
                cs.append(time.perf_counter() - t)
                s2 = e.stats()
                # the call's kernels minus those of the same Check on its own (whichever path it takes: its seed / walk / finalize launches are in both)
                km.append((s1["kernel_ms"] - s0["kernel_ms"]) - (s2["kernel_ms"] - s1["kernel_ms"]))
                compared += it.size
                mism += int((p != cp).sum() + (er != ce).sum() + (fl != aclgpu.EXPLAIN_WITNESS).sum())
                broken += chains(it, off, hops)
                hop_n += np.diff(off.astype(np.int64)).tolist()
            for k in range(min(reps, 3 if n >= 4096 else reps) + 1):
                t = time.perf_counter()
                e.lookup_subjects_ids_batch("pod", "view", "user", "", pods if n > 1 else pods[:1])
                ls.append(time.perf_counter() - t)
            res["calls"][str(n)] = {"explain_p50_us": pct(xs[2:], 50), "explain_p99_us": pct(xs[2:], 99), "explain_kernel_us": round(float(np.mean(km[2:])) * 1e3, 1),
                                    "check_p50_us": pct(cs[2:], 50), "lookup_subjects_p50_us": pct(ls[1:], 50), "hops_mean": round(float(np.mean(hop_n)), 2),
                                    "hops_max": int(np.max(hop_n))}
        res["answers_compared"], res["mismatches"], res["broken_chains"] = compared, mism, broken
        res["overflow_retries"] = int(e.stats()["overflow_retries"] - r0)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if a.md:
        write_md(res, a.md)
    return 0 if mism == 0 and broken == 0 else 1


if __name__ == "__main__":
    sys.exit(main())

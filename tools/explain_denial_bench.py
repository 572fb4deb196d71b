"""Explain for denials on C4 (1 M objects, 100 000 users, 5-level nested groups at scale 1.0): profiles/explain_denial_c4.{json,md}.

Denied `pod#view` items: the pods of the workload's Check stream with the largest closures of holders (about 22 400 users a pod at scale 1.0), each asked
for a user outside its closure.  For 1, 64 and 4 096 items, once about DISTINCT pods and once about ONE shared pod, in one process on one snapshot:
  acl_explain_denial_bulk_ids   call p50 / p99 and the time of k_reach_local inside it (acl_set_timing: the call's kernel time minus the kernel time of the
                                same Check called on its own)
  acl_check_bulk_ids            of the same items (what the denial's explanation adds is the difference)
  acl_lookup_subjects_batch     of the same pods: the same walk, which also emits every subject row it reaches
The whole measurement runs three times; the spread of a figure is the distance between the least and the largest of its three p50s.  Every timed answer is
compared with Check's; the grants are checked here for their shape only (sorted, distinct, levels 1..50) -- tests/test_explain_denial_gpu.py holds the
grants themselves to the oracles.  No speed bar: the figures are recorded.

  python tools/explain_denial_bench.py --out profiles/explain_denial_c4.json --md profiles/explain_denial_c4.md     (on a box with the GPU; --quick: fewer calls)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "spicedb-kubeapi-proxy_amd"))

ROUNDS = 3


def pct(xs, q):
    return round(float(np.percentile(np.asarray(xs) * 1e6, q)), 1)


def misshapen(off, grants):
    """items whose grants are not sorted by (level, rtype, relation, rid), not distinct, or carry a level outside 1..50"""
    bad = 0
    for i in range(off.size - 1):
        g = grants[off[i]:off[i + 1]]
        keys = list(zip(g["level"].tolist(), g["rtype"].tolist(), g["relation"].tolist(), g["rid"].tolist()))
        ok = keys == sorted(keys) and len({k[1:] for k in keys}) == len(keys) and all(1 <= k[0] <= 50 for k in keys)
        bad += int(not ok)
    return bad


def write_md(res, path):
    out = ["# Explain for denials on C4: call time next to Check and LookupSubjects", "",
           f"`tools/explain_denial_bench.py` on one MI355X, C4 at scale {res['scale']} ({res['relationships']} relationships): denied `pod#view` items on the",
           f"pods with the largest closures of the workload's Check stream ({res['holders_mean']} holders a pod on average, {res['holders_max']} at most), for users",
           "outside them.  One process, one snapshot.  `kernel` is the call's event-timed kernel time (`acl_set_timing`) minus that of the same Check",
           "called on its own; the other columns are host wall-clock times of whole calls.  `LookupSubjects` walks the same pods (one pod where the",
           f"items share one).  Every figure is the median of the {res['rounds']} rounds' figures; `spread` is the distance between the least and the largest",
           "of the rounds' denial p50s.", "",
           "| items | pods | denial p50 us | spread us | denial p99 us | kernel us (mean) | Check p50 us | LookupSubjects p50 us | grants per item (mean / max) |",
           "|---|---|---|---|---|---|---|---|---|"]
    for name, c in res["calls"].items():
        out.append(f"| {c['items']} | {c['pods']} | {c['denial_p50_us']} | {c['denial_p50_spread_us']} | {c['denial_p99_us']} | {c['denial_kernel_us']} | {c['check_p50_us']} | "
                   f"{c['lookup_subjects_p50_us']} | {c['grants_mean']} / {c['grants_max']} |")
    out += ["", f"First call on the snapshot: {res['first_call_ms']} ms (it builds and uploads the subject rows, whose visited-bit layout the walk uses).",
            f"Answers compared with Check: {res['answers_compared']}, mismatches: {res['mismatches']}; items with misshapen grants: {res['misshapen']}; "
            f"log / region overflow retries during the timed calls: {res['overflow_retries']}.", ""]
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
    res = {"workload": "C4", "scale": a.scale, "relationships": w.ntuples, "rounds": ROUNDS, "calls": {}}
    with aclgpu.Engine(w.schema, device=0) as e:
        w.load(e)
        # the stream's distinct pods, each asked for a user drawn at random: most of them are denied (the stream's own pairs are mostly granted)
        _, first = np.unique(w.res, return_index=True)
        pods = w.res[np.sort(first)]
        users = np.random.default_rng(7).integers(0, e.object_count("user"), size=pods.size).astype(np.uint32)
        stream = e.make_items("pod", "view", pods, "user", "", users)
        perm, err = e.check_bulk_ids(stream)  # (builds the forward snapshot)
        denied = stream[(perm == aclgpu.PERM_NO) & (err == 0)]  # one denied item per distinct pod
        res["load_s"] = round(time.perf_counter() - t0, 2)
        t = time.perf_counter()
        e.explain_denial_ids(denied[:1])
        res["first_call_ms"] = round((time.perf_counter() - t) * 1e3, 2)
        # the pods with the largest closures first
        holders = np.zeros(denied.size, dtype=np.uint64)  # (of every candidate pod; the 4 096 largest are kept)
        for b in range(0, denied.size, 256):
            _bm, cnt, _fl = e.lookup_subjects_ids_batch("pod", "view", "user", "", denied["resource_id"][b:b + 256])
            holders[b:b + 256] = cnt
        order = np.argsort(-holders.astype(np.int64), kind="stable")
        denied, holders = denied[order][:4096], holders[order][:4096]
        res["holders_mean"], res["holders_max"] = int(holders.mean()), int(holders.max())
        # one shared pod: the largest closure, and users outside it
        bm, _cnt, _fl = e.lookup_subjects_ids_batch("pod", "view", "user", "", denied["resource_id"][:1])
        inside = np.unpackbits(bm[0].view(np.uint8), bitorder="little")[:e.object_count("user")].astype(bool)
        outside = np.flatnonzero(~inside)[:4096].astype(np.uint32)
        shared = e.make_items("pod", "view", np.full(outside.size, denied["resource_id"][0], dtype=np.uint32), "user", "", outside)
        r0 = e.stats()["overflow_retries"]
        e.set_timing(True)
        mism = bad = compared = 0
        cases = [(f"{n} distinct", denied[:n], n) for n in (1, 64, 4096) if n <= denied.size] + [(f"{n} shared", shared[:n], 1) for n in (64, 4096) if n <= shared.size]
        for name, items, npods in cases:
            n = items.size
            reps = (3 if a.quick else 20) if n < 4096 else (2 if a.quick else 6)
            pods = np.ascontiguousarray(np.unique(items["resource_id"]))
            rounds = []
            gn = []
            for _round in range(ROUNDS):
                xs, cs, ls, km = [], [], [], []
                for k in range(reps + 2):
                    it = items if n > 1 else denied[k % 64:k % 64 + 1]
                    s0 = e.stats()
                    t = time.perf_counter()
                    p, er, fl, off, grants = e.explain_denial_ids(it)
                    xs.append(time.perf_counter() - t)
                    s1 = e.stats()
                    t = time.perf_counter()
                    cp, ce = e.check_bulk_ids(it)
                    cs.append(time.perf_counter() - t)
                    s2 = e.stats()
                    km.append((s1["kernel_ms"] - s0["kernel_ms"]) - (s2["kernel_ms"] - s1["kernel_ms"]))
                    compared += it.size
                    mism += int((p != cp).sum() + (er != ce).sum() + (fl != aclgpu.EXPLAIN_DENIAL).sum())
                    if k == 0:
                        bad += misshapen(off, grants)
                        gn = np.diff(off.astype(np.int64)).tolist()
                for k in range(min(reps, 3 if n >= 4096 else reps) + 1):
                    lp = pods if n > 1 else denied["resource_id"][k % 64:k % 64 + 1]
                    t = time.perf_counter()
                    e.lookup_subjects_ids_batch("pod", "view", "user", "", lp)
                    ls.append(time.perf_counter() - t)
                rounds.append({"denial_p50_us": pct(xs[2:], 50), "denial_p99_us": pct(xs[2:], 99), "denial_kernel_us": round(float(np.mean(km[2:])) * 1e3, 1),
                               "check_p50_us": pct(cs[2:], 50), "lookup_subjects_p50_us": pct(ls[1:], 50)})
            med = {k: round(float(np.median([r[k] for r in rounds])), 1) for k in rounds[0]}
            p50s = [r["denial_p50_us"] for r in rounds]
            res["calls"][name] = dict(med, items=int(n), pods=int(pods.size if n > 1 else 1), denial_p50_spread_us=round(max(p50s) - min(p50s), 1), rounds=rounds,
                                      grants_mean=round(float(np.mean(gn)), 1), grants_max=int(np.max(gn)))
        res["answers_compared"], res["mismatches"], res["misshapen"] = compared, mism, bad
        res["overflow_retries"] = int(e.stats()["overflow_retries"] - r0)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if a.md:
        write_md(res, a.md)
    return 0 if mism == 0 and bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())

"""Explain for revocation on C4 (1 M objects, 100 000 users, 5-level nested groups at scale 1.0): profiles/explain_revoke_c4.{json,md}.

Granted `pod#view` items of the workload's Check stream, 1, 64 and 4 096 items a call, in one process on one snapshot:
  acl_explain_revoke_bulk_ids   call p50 / p99 and the time of k_revoke_local inside it (acl_set_timing: the call's kernel time minus the kernel time of
                                acl_explain_bulk_ids of the same items called on its own -- the same Check and the same witness walk)
  acl_explain_bulk_ids          of the same items (what the cuts add is the difference)
  the write route               the only way to the same answer without the call, one item at a time: Explain for a witness, then per hop acl_write DELETE,
                                Check, acl_write TOUCH -- every Check pays the snapshot patch of the write before it -- and one more Explain, which pays the
                                last patch and the rebuild of the subject rows.  Its answer (the hops whose delete turned the Check) is compared with the call's.
The whole measurement runs three times; the spread of a figure is the distance between the least and the largest of its three p50s.  Every timed answer is
compared with Check's; tests/test_explain_revoke_gpu.py holds the cuts themselves to the oracles.  No speed bar: the figures are recorded.

  python tools/explain_revoke_bench.py --out profiles/explain_revoke_c4.json --md profiles/explain_revoke_c4.md     (on a box with the GPU; --quick: fewer calls)"""
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
ROUTE_ITEMS = 16


def pct(xs, q):
    return round(float(np.percentile(np.asarray(xs) * 1e6, q)), 1)


def write_md(res, path):
    out = ["# Explain for revocation on C4: call time next to Explain and to the write route", "",
           f"`tools/explain_revoke_bench.py` on one MI355X, C4 at scale {res['scale']} ({res['relationships']} relationships): granted `pod#view` items of the",
           "workload's Check stream.  One process, one snapshot.  `kernel` is the call's event-timed kernel time (`acl_set_timing`) minus that of",
           "`acl_explain_bulk_ids` of the same items called on its own, which leaves `k_revoke_local`; the other columns are host wall-clock times of whole calls.",
           f"Every figure is the median of the {res['rounds']} rounds' figures; `spread` is the distance between the least and the largest of the rounds' p50s.", "",
           "| items | revoke p50 us | spread us | revoke p99 us | k_revoke_local us (mean) | Explain p50 us | masked walks per call | hops per item (mean / max) | cuts per item (mean / max) | items without a cut |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for c in res["calls"].values():
        out.append(f"| {c['items']} | {c['revoke_p50_us']} | {c['revoke_p50_spread_us']} | {c['revoke_p99_us']} | {c['revoke_kernel_us']} | {c['explain_p50_us']} | {c['walks']} | "
                   f"{c['hops_mean']} / {c['hops_max']} | {c['cuts_mean']} / {c['cuts_max']} | {c['no_cut']} |")
    r = res["route"]
    out += ["", "## One item: the call next to the write route", "",
            f"{r['items']} items, each asked on its own.  The route is Explain, then per witness hop `acl_write` DELETE, Check, `acl_write` TOUCH, then one more Explain",
            "(the read that pays for the last write: its snapshot patch and the rebuild of the subject rows).  It changes the live store and the snapshot",
            f"{r['writes_mean']} times an item; the call changes nothing.", "",
            "| | p50 us | p99 us |", "|---|---|---|",
            f"| acl_explain_revoke_bulk_ids, one item | {r['call_p50_us']} | {r['call_p99_us']} |",
            f"| the write route, one item | {r['route_p50_us']} | {r['route_p99_us']} |",
            f"| ... of which the closing Explain | {r['closing_p50_us']} | {r['closing_p99_us']} |", "",
            f"Cut sets compared between the route and the call: {r['compared']}, mismatches: {r['mismatches']}.", "",
            "## Where the call loses", "",
            "The call launches one block per (item, distinct hop) where Explain launches one per item, and a walk that does NOT find the subject has no early",
            "exit: it runs the closure dry.  A hop that is no cut costs a walk up to the level at which the next chain is found, and an item whose grant is",
            f"redundant pays such a walk for every hop.  Of the 4 096 items here {res['calls'].get('4096', {}).get('no_cut', 'n/a')} have no cut at all.  Measured: one item costs {res['calls']['1']['revoke_over_explain']} times an",
            f"Explain of the same item, 4 096 items {res['calls'].get('4096', res['calls']['1'])['revoke_over_explain']} times ({res['calls'].get('4096', res['calls']['1'])['walks']} masked walks, "
            f"{res['calls'].get('4096', res['calls']['1'])['revoke_kernel_us']} us of `k_revoke_local`).  The row of one item shows the figures of the 64",
            "different items its single calls were drawn from.", "",
            f"First call on the snapshot: {res['first_call_ms']} ms (it builds and uploads the subject rows).  Answers compared with Check: {res['answers_compared']}, "
            f"mismatches: {res['mismatches']}; log overflow retries during the timed calls: {res['overflow_retries']}.", ""]
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
    prefix = {"user": "user-", "group": "group-", "namespace": "ns-", "pod": "pod-"}
    with aclgpu.Engine(w.schema, device=0) as e:
        # names for every object, so that the write route can name a hop (dense ids follow interning order: name k is id k of the bulk load)
        for t, p in prefix.items():
            for k in range(w.nobjects[t]):
                e.intern(t, f"{p}{k}")
        w.load(e)
        tname = {e.type_id(t): t for t in prefix}
        rname = {(e.type_id(t), e.relation_id(t, m)): m for t, ms in (("group", ["member"]), ("namespace", ["viewer", "creator"]), ("pod", ["namespace", "viewer", "creator"])) for m in ms}
        stream = e.make_items("pod", "view", w.res, "user", "", w.subj)
        perm, err = e.check_bulk_ids(stream)  # (builds the forward snapshot)
        granted = stream[(perm == aclgpu.PERM_HAS) & (err == 0)]
        _, first = np.unique(granted.view(np.dtype((np.void, granted.dtype.itemsize))), return_index=True)
        granted = granted[np.sort(first)][:4096]
        res["load_s"] = round(time.perf_counter() - t0, 2)
        t = time.perf_counter()
        e.explain_revoke_ids(granted[:1])
        res["first_call_ms"] = round((time.perf_counter() - t) * 1e3, 2)
        r0 = e.stats()["overflow_retries"]
        e.set_timing(True)
        mism = compared = 0
        for n in [n for n in (1, 64, 4096) if n <= granted.size]:
            items = granted[:n]
            reps = (3 if a.quick else 20) if n < 4096 else (2 if a.quick else 6)
            rounds = []
            hn = cn = []
            for _round in range(ROUNDS):
                xs, es, km = [], [], []
                for k in range(reps + 2):
                    it = items if n > 1 else granted[k % 64:k % 64 + 1]
                    s0 = e.stats()
                    t = time.perf_counter()
                    p, er, fl, off, cuts = e.explain_revoke_ids(it)
                    xs.append(time.perf_counter() - t)
                    s1 = e.stats()
                    t = time.perf_counter()
                    xp, xer, xfl, xoff, hops = e.explain_ids(it)
                    es.append(time.perf_counter() - t)
                    s2 = e.stats()
                    km.append((s1["kernel_ms"] - s0["kernel_ms"]) - (s2["kernel_ms"] - s1["kernel_ms"]))
                    cp, ce = e.check_bulk_ids(it)
                    compared += it.size
                    mism += int((p != cp).sum() + (er != ce).sum() + (fl != aclgpu.EXPLAIN_REVOKE).sum() + (xfl != aclgpu.EXPLAIN_WITNESS).sum())
                    if k == 0 and n > 1:
                        hn, cn = np.diff(xoff.astype(np.int64)), np.diff(off.astype(np.int64))
                        mism += int((cn > hn).sum())
                if n == 1:  # (the single calls walk 64 different items: their figures are those of the first 64 asked at once)
                    _p, _e, _f, off, _c = e.explain_revoke_ids(granted[:64])
                    hn, cn = np.diff(e.explain_ids(granted[:64])[3].astype(np.int64)), np.diff(off.astype(np.int64))
                rounds.append({"revoke_p50_us": pct(xs[2:], 50), "revoke_p99_us": pct(xs[2:], 99), "revoke_kernel_us": round(float(np.mean(km[2:])) * 1e3, 1),
                               "explain_p50_us": pct(es[2:], 50)})
            med = {k: round(float(np.median([r[k] for r in rounds])), 1) for k in rounds[0]}
            p50s = [r["revoke_p50_us"] for r in rounds]
            res["calls"][str(n)] = dict(med, items=int(n), revoke_p50_spread_us=round(max(p50s) - min(p50s), 1), rounds=rounds, walks=int(hn.sum()) if n > 1 else round(float(hn.mean()), 1),
                                        hops_mean=round(float(hn.mean()), 2), hops_max=int(hn.max()), cuts_mean=round(float(cn.mean()), 2), cuts_max=int(cn.max()),
                                        no_cut=int((cn == 0).sum()), revoke_over_explain=round(med["revoke_p50_us"] / max(med["explain_p50_us"], 1e-9), 1))
        res["answers_compared"], res["mismatches"] = compared, mism
        res["overflow_retries"] = int(e.stats()["overflow_retries"] - r0)
        # ---- one item at a time: the call, and the write route on the live store
        e.set_timing(False)

        def named(h):
            rt, st = tname[int(h["rtype"])], tname[int(h["stype"])]
            return (rt, f"{prefix[rt]}{int(h['rid'])}", rname[(int(h["rtype"]), int(h["relation"]))], st, f"{prefix[st]}{int(h['sid'])}", "" if int(h["srel"]) == 0xFFFF else "member")

        key = lambda h: (int(h["rtype"]), int(h["relation"]), int(h["rid"]), int(h["stype"]), int(h["srel"]), int(h["sid"]))  # noqa: E731
        calls, routes, closing, writes = [], [], [], []
        rcomp = rmism = 0
        for k in range(min(ROUTE_ITEMS, granted.size) + 1):
            it = granted[k:k + 1]
            t = time.perf_counter()
            _p, _e, _f, _off, cuts = e.explain_revoke_ids(it)
            calls.append(time.perf_counter() - t)
            want = {key(h) for h in cuts}
            t = time.perf_counter()
            _p, _e, _f, _off, hops = e.explain_ids(it)
            got, nw, seen = set(), 0, set()
            for h in hops:
                if key(h) in seen:
                    continue
                seen.add(key(h))
                rel = named(h)
                e.write([(aclgpu.OP_DELETE, rel)])
                cp, ce = e.check_bulk_ids(it)
                if int(cp[0]) != aclgpu.PERM_HAS or int(ce[0]):
                    got.add(key(h))
                e.write([(aclgpu.OP_TOUCH, rel)])
                nw += 2
            t1 = time.perf_counter()
            e.explain_ids(it)
            t2 = time.perf_counter()
            routes.append(t2 - t)
            closing.append(t2 - t1)
            writes.append(nw)
            rcomp += 1
            rmism += int(got != want)
        res["route"] = {"items": len(calls) - 1, "call_p50_us": pct(calls[1:], 50), "call_p99_us": pct(calls[1:], 99), "route_p50_us": pct(routes[1:], 50),
                        "route_p99_us": pct(routes[1:], 99), "closing_p50_us": pct(closing[1:], 50), "closing_p99_us": pct(closing[1:], 99),
                        "writes_mean": round(float(np.mean(writes[1:])), 1), "compared": rcomp, "mismatches": rmism}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if a.md:
        write_md(res, a.md)
    return 0 if mism == 0 and rmism == 0 else 1


if __name__ == "__main__":
    sys.exit(main())

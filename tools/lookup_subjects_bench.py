"""LookupSubjects on C4 (1 M objects, 100 000 users, 5-level nested groups at scale 1.0): one JSON line.

  single-resource latency (p50 / p99) of the id form (acl_lookup_subjects_batch, n = 1) and of the string form (acl_lookup_subjects),
  over pods drawn by C4's request mix (workloads.c4: the Check stream's resources);
  lookups/s with 64 and 256 resources per call;
  the subject rows' build + upload (the first call's extra time over a steady call) and their bytes (acl_stats.snapshot_bytes, before / after);
  the brute-force alternative for the same resources: one acl_check_bulk_ids of R x every user per resource, timed in the same process.
Every timed answer is compared with that brute-force row (mismatches are counted and reported).  Kernel times: run this under
`rocprofv3 --kernel-trace --stats` separately (--quick keeps such a run short).

--shards N: the same pods through N LOGICAL shards of one device (acl_shard_subjects_bulk over the in-process ThreadNative communicator: emulated, not a
measurement of N > 1 hardware) -- per call of 1, 64 and 256 pods: p50 / p99, levels, exchanges, exchanged bytes, host syncs; the unsharded
acl_lookup_subjects_batch on the same pods in the same command as the baseline; every timed answer compared with the unsharded rows.

How profiles/lookup_subjects_sharded.{json,md} are made (on a box with the GPU):
  python tools/lookup_subjects_bench.py --shards 2 --out profiles/lookup_subjects_sharded.json
  python tools/lookup_subjects_bench.py --shards 8 --out profiles/lookup_subjects_sharded.json --append
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o subj -- python tools/lookup_subjects_bench.py --shards 2 --quick     (a run of its own)
  python tools/lookup_subjects_bench.py --kernel-stats DIR/.../subj_kernel_stats.csv --json profiles/lookup_subjects_sharded.json --md profiles/lookup_subjects_sharded.md
The last step needs no GPU: it turns the JSON lines and the profiler's per-kernel table into the markdown note (every figure under the label
"logical shards on one device: emulated, unmeasured on N > 1 hardware")."""
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
    return float(np.percentile(np.asarray(xs) * 1e6, q)) if len(xs) else None


def ids_of(row):
    return np.flatnonzero(np.unpackbits(np.ascontiguousarray(row, dtype=np.uint32).view(np.uint8), bitorder="little"))


LABEL = "logical shards on one device: emulated, unmeasured on N > 1 hardware"


def write_md(a):
    """the markdown note from the tool's JSON lines (--json) and a rocprofv3 *_kernel_stats.csv (--kernel-stats); no GPU needed"""
    import csv
    runs = [json.loads(x) for x in open(a.json) if x.strip().startswith("{")]
    out = ["# LookupSubjects through the sharded native loop on C4: " + LABEL, "",
           "`tools/lookup_subjects_bench.py --shards N` on one MI355X: N engines as N logical shards of the one device, the collectives an in-process copy",
           "between them (ThreadNative, driven from Python threads) -- the loop, the kernels and the decisions are the ones RCCL drives, the times are not",
           "those of N GPUs.  The unsharded `acl_lookup_subjects_batch` on the same pods, timed in the same command, is the baseline, not a target.", ""]
    for r in runs:
        out += [f"## {r['shards']} logical shards, scale {r['scale']} ({LABEL})", "",
                "| pods per call | p50 us | p99 us | unsharded p50 us | unsharded p99 us | levels | exchanges | with entries | exchanged bytes | entries | host syncs | retries |",
                "|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for n, c in r["calls"].items():
            out.append(f"| {n} | {c['p50_us']} | {c['p99_us']} | {c['unsharded_p50_us']} | {c['unsharded_p99_us']} | {c['levels']} | {c['exchanges']} | {c['data_exchanges']} | "
                       f"{c['exchanged_bytes']} | {c['entries_exchanged']} | {c['host_syncs']} | {c['retries']} |")
        out += ["", f"Answers compared with the unsharded rows: {r['answers_compared']}, mismatches: {r['mismatches']}.", ""]
    if a.kernel_stats:
        out += ["## Kernels (`rocprofv3 --kernel-trace --stats -- python tools/lookup_subjects_bench.py --shards 2 --quick`, a run of its own; " + LABEL + ")", "",
                "| kernel | calls | total us | mean us | min us | max us |", "|---|---|---|---|---|---|"]
        for row in csv.DictReader(open(a.kernel_stats)):
            g = lambda *ks: next((row[k] for k in ks if k in row), "0")  # noqa: E731
            us = lambda v: round(float(v) / 1e3, 2)  # noqa: E731
            out.append(f"| `{g('Name', 'KernelName')}` | {g('Calls')} | {us(g('TotalDurationNs'))} | {us(g('AverageNs'))} | {us(g('MinNs'))} | {us(g('MaxNs'))} |")
        out.append("")
    with open(a.md, "w") as f:
        f.write("\n".join(out))
    return 0


def main_sharded(a):
    import aclgpu
    from aclgpu import sharded, workloads

    reps = 5 if a.quick else 30
    w = workloads.c4(scale=a.scale, batch=4096)
    pods = np.array(list(dict.fromkeys(w.res.tolist())), dtype=np.uint32)[:256]
    sizes = [n for n in (1, 64, 256) if n <= pods.size]
    res = {"workload": "C4", "scale": a.scale, "shards": a.shards, "label": LABEL, "calls": {}}
    # ---- the baseline: the unsharded single-launch walk on the same pods, same box
    with aclgpu.Engine(w.schema, device=0) as e:
        w.load(e)
        want, _, _ = e.lookup_subjects_ids_batch("pod", "view", "user", "", pods)
        for n in sizes:
            ts = []
            for _ in range(reps + 2):
                t = time.perf_counter()
                e.lookup_subjects_ids_batch("pod", "view", "user", "", pods[:n])
                ts.append(time.perf_counter() - t)
            res["calls"][str(n)] = {"unsharded_p50_us": round(pct(ts[2:], 50), 1), "unsharded_p99_us": round(pct(ts[2:], 99), 1)}
    engines = []

    def make(rank, world):
        e = aclgpu.Engine(w.schema, contexts=1)
        w.load(e)
        engines.append(e)
        return sharded.GpuShard(e, rank, world)

    def run(se):
        out = {}
        for n in sizes:
            ts, mism, stats = [], 0, None
            for k in range(reps + 2):
                se.comm.barrier()  # (every rank starts the call together: the time is the call's, not the wait for the slowest rank's previous one)
                t = time.perf_counter()
                bm, flags, _x, stats = se.lookup_subjects_ids_batch_native("pod", "view", "user", "", pods[:n])
                ts.append(time.perf_counter() - t)
                got = bm.cpu().numpy().view(np.uint32)
                mism += int(not np.array_equal(got[:, :want.shape[1]], want[:n]) or bool(flags.any()))
            out[n] = (ts[2:], mism, stats)
        return out

    try:
        outs = sharded.run_logical_shards(a.shards, make, run)
    finally:
        for e in engines:
            e.close()
    mism = 0
    for n in sizes:
        ts = np.max(np.array([o[n][0] for o in outs]), axis=0)  # a call ends when its slowest rank returns
        st = outs[0][n][2]
        mism += sum(o[n][1] for o in outs)
        res["calls"][str(n)].update({"p50_us": round(pct(ts, 50), 1), "p99_us": round(pct(ts, 99), 1), "levels": st["levels"], "exchanges": st["exchanges"],
                                     "data_exchanges": st["data_exchanges"], "exchanged_bytes": st["exchanged_bytes"], "entries_exchanged": st["entries_exchanged"],
                                     "host_syncs": st["host_syncs"], "retries": st["retries"]})
    res["answers_compared"] = a.shards * sum(reps + 2 for _ in sizes)
    res["mismatches"] = mism
    res["kernel_times"] = "a separate rocprofv3 --kernel-trace --stats run (this file's docstring); --kernel-stats puts its table into the .md"
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a" if a.append else "w") as f:
            f.write(line + "\n")
    return 0 if mism == 0 else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--singles", type=int, default=200, help="single-resource calls per form")
    ap.add_argument("--quick", action="store_true", help="fewer calls (profiler runs)")
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    ap.add_argument("--shards", type=int, default=0, help="N > 0: the same pods through N logical shards of this device (the native sharded loop), with the unsharded call as the baseline")
    ap.add_argument("--append", action="store_true", help="append to --out instead of overwriting it")
    ap.add_argument("--kernel-stats", default="", help="a rocprofv3 *_kernel_stats.csv: with --json and --md, write the markdown note (no GPU needed)")
    ap.add_argument("--json", default="", help="the file of JSON lines --shards runs wrote (input of --md)")
    ap.add_argument("--md", default="", help="write the markdown note of the --shards runs here")
    a = ap.parse_args()
    if a.md:
        return write_md(a)
    if a.shards > 0:
        return main_sharded(a)
    import aclgpu
    from aclgpu import workloads

    singles = 24 if a.quick else a.singles
    t0 = time.perf_counter()
    w = workloads.c4(scale=a.scale, batch=max(4096, singles * 4))
    res = {"workload": "C4", "scale": a.scale}
    with aclgpu.Engine(w.schema, device=0) as e:
        # names first (dense ids follow interning order, so name k is id k of the bulk load): pods `ns<namespace>/pod-<id>`, users `user-<id>`
        pod_ns = np.zeros(w.nobjects["pod"], dtype=np.int64)
        for e_ in w.edges:
            if e_[0] == "pod" and e_[1] == "namespace":
                pod_ns[e_[4]] = e_[5]
        for k in range(w.nobjects["pod"]):
            e.intern("pod", f"ns{int(pod_ns[k])}/pod-{k}")
        for k in range(w.nobjects["user"]):
            e.intern("user", f"user-{k}")
        w.load(e)
        nuser = e.object_count("user")
        # the forward snapshot first (a Check), so that the first LookupSubjects pays for the subject rows only
        e.check_bulk_ids(e.make_items("pod", "view", w.res[:16], "user", "", w.subj[:16]))
        res["load_s"] = round(time.perf_counter() - t0, 2)
        pods = np.array(list(dict.fromkeys(w.res.tolist())), dtype=np.uint32)[:max(singles, 256)]
        b0 = e.stats()["snapshot_bytes"]
        t = time.perf_counter()
        first, _, _ = e.lookup_subjects_ids_batch("pod", "view", "user", "", pods[:1])
        first_s = time.perf_counter() - t
        res["subject_rows_bytes"] = int(e.stats()["snapshot_bytes"] - b0)

        # brute force: R x every user, one bulk Check per resource (and the reference rows every answer is compared with)
        subj = np.arange(nuser, dtype=np.uint32)
        want, brute = {}, []
        for r in pods[:singles]:
            items = e.make_items("pod", "view", np.full(nuser, r, dtype=np.uint32), "user", "", subj)
            t = time.perf_counter()
            perm, _ = e.check_bulk_ids(items)
            brute.append(time.perf_counter() - t)
            want[int(r)] = np.flatnonzero(perm == aclgpu.PERM_HAS)
        for r in pods[singles:]:
            perm, _ = e.check_bulk_ids(e.make_items("pod", "view", np.full(nuser, r, dtype=np.uint32), "user", "", subj))
            want[int(r)] = np.flatnonzero(perm == aclgpu.PERM_HAS)
        mism = int(not np.array_equal(ids_of(first[0]), want[int(pods[0])]))

        ids_t, str_t = [], []
        names = [e.object_name("pod", int(r)) for r in pods[:singles]]
        for _ in range(3):  # warm-up
            e.lookup_subjects_ids_batch("pod", "view", "user", "", pods[:1])
            e.lookup_subjects_bitmap("pod", names[0], "view", "user", want_excluded=False)
        for i, r in enumerate(pods[:singles]):
            t = time.perf_counter()
            bm, _, _ = e.lookup_subjects_ids_batch("pod", "view", "user", "", pods[i:i + 1])
            ids_t.append(time.perf_counter() - t)
            mism += int(not np.array_equal(ids_of(bm[0]), want[int(r)]))
            t = time.perf_counter()
            row, _, _, _ = e.lookup_subjects_bitmap("pod", names[i], "view", "user", want_excluded=False)
            str_t.append(time.perf_counter() - t)
            mism += int(not np.array_equal(ids_of(row), want[int(r)]))
        res["single_ids_p50_us"], res["single_ids_p99_us"] = round(pct(ids_t, 50), 1), round(pct(ids_t, 99), 1)
        res["single_string_p50_us"], res["single_string_p99_us"] = round(pct(str_t, 50), 1), round(pct(str_t, 99), 1)
        res["brute_force_p50_us"], res["brute_force_p99_us"] = round(pct(brute, 50), 1), round(pct(brute, 99), 1)
        res["subject_rows_build_upload_ms"] = round((first_s - float(np.median(ids_t))) * 1e3, 2)
        for batch in (64, 256):
            rs = pods[:batch]
            e.lookup_subjects_ids_batch("pod", "view", "user", "", rs)
            reps = 2 if a.quick else 10
            t = time.perf_counter()
            for _ in range(reps):
                bms, counts, _ = e.lookup_subjects_ids_batch("pod", "view", "user", "", rs)
            dt = (time.perf_counter() - t) / reps
            res[f"lookups_per_s_{batch}"] = round(batch / dt, 1)
            for i, r in enumerate(rs):
                mism += int(not np.array_equal(ids_of(bms[i]), want[int(r)]))
        res["mean_subjects_per_pod"] = round(float(np.mean([want[int(r)].size for r in pods[:singles]])), 1)
        res["answers_compared"] = singles * 2 + 1 + 64 + 256
        res["mismatches"] = mism
        res["kernel_times"] = "not measured here (rocprofv3 --kernel-trace --stats run)"
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if mism == 0 else 1


if __name__ == "__main__":
    sys.exit(main())

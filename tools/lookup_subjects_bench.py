"""LookupSubjects on C4 (1 M objects, 100 000 users, 5-level nested groups at scale 1.0): one JSON line.

  single-resource latency (p50 / p99) of the id form (acl_lookup_subjects_batch, n = 1) and of the string form (acl_lookup_subjects),
  over pods drawn by C4's request mix (workloads.c4: the Check stream's resources);
  lookups/s with 64 and 256 resources per call;
  the subject rows' build + upload (the first call's extra time over a steady call) and their bytes (acl_stats.snapshot_bytes, before / after);
  the brute-force alternative for the same resources: one acl_check_bulk_ids of R x every user per resource, timed in the same process.
Every timed answer is compared with that brute-force row (mismatches are counted and reported).  Kernel times: run this under
`rocprofv3 --kernel-trace --stats` separately (--quick keeps such a run short)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--singles", type=int, default=200, help="single-resource calls per form")
    ap.add_argument("--quick", action="store_true", help="fewer calls (profiler runs)")
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    a = ap.parse_args()
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

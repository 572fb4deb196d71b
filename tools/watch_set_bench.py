"""Watch sets on C4 (scale 1.0) and on the 100 M-relationship replica (C5's graph on one device, `--workload c5r`): what a poll costs, and what the same
answer costs the way a caller gets it today.

Per W in --watchers (1, 64, 1 024 watchers on pod#view), one group-membership write per step (a TOUCH or the DELETE of a `group#member@user`
relationship of one of the watchers: no update of type pod exists, the reference's watch hears nothing):
  poll        p50 / p99 (the maximum, below 100 steps) of acl_watch_set_poll (the snapshot patch of the step's write is inside, as it is inside the alternative's first read);
  kernels     HIP-event time per poll of everything the poll launches, and of it the reverse walk (acl_stats kernel_ms / rev_local_ms with
              acl_set_timing on, in a second pass of the same run: event records would otherwise sit inside the timed polls) -- the rest is the diff;
  alternative acl_lookup_resources_batch of the W subjects into pinned rows (acl_host_alloc) + a numpy XOR against the previous rows + flatnonzero of
              the changed words, same box, same run, same writes (every step: write, poll, alternative).
Both must give the same changes at every step (asserted; a mismatch ends the run with a non-zero status).
A set holds at most 1 GiB of rows: where W watchers do not fit one set (the replica's 1 MB rows) they are spread over several and polled in turn.

Repetition: --warmup steps are thrown away, then --steps timed steps per W; the run is repeated --repeat times in ONE process on one engine and the
JSON keeps every repetition's p50 so that the spread is visible; quote the median repetition.

  python tools/watch_set_bench.py --workload c4  --out profiles/watch_set_c4
  python tools/watch_set_bench.py --workload c5r --out profiles/watch_set_c5r
write <out>.json (one JSON document) and <out>.md (the table)."""
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
    return round(float(np.percentile(np.asarray(xs) * 1e6, q)), 1) if len(xs) else None


def changes_by_xor(x, cur, watcher_ids):
    """the alternative's diff on the host (x = previous rows ^ cur): (watcher, resource id, gained) sorted by (watcher, resource id)"""
    rows, words = np.nonzero(x)
    out = []
    for r, wd in zip(rows.tolist(), words.tolist()):
        v, nv = int(x[r, wd]), int(cur[r, wd])
        while v:
            b = (v & -v).bit_length() - 1
            out.append((watcher_ids[r], wd * 32 + b, (nv >> b) & 1))
            v &= v - 1
    return sorted(out)


def write_out(res, out):
    """<out>.json and <out>.md from the result document (also after every W: a run that is cut short leaves what it had)"""
    with open(out + ".json", "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    mism = res.get("mismatches", 0)
    tail = "p99" if res["steps"] >= 100 else f"max of {res['steps']}"  # (fewer than 100 samples have no 99th percentile: the column is their maximum)
    md = [f"# Watch sets on {res['workload'].upper()} (scale {res['scale']}: {res['relationships']} relationships, {res['pods']} pods)", "",
          "`tools/watch_set_bench.py`: one group-membership write per step, then the set's poll and -- same run, same writes -- the alternative a caller",
          "has without watch sets: `acl_lookup_resources_batch` of the W subjects into pinned rows + a numpy XOR against the previous rows.",
          f"{res['steps']} timed steps after {res['warmup']} warm-up steps, {res.get('repeat', 3)} repetitions in one process; every row is ONE repetition, the one",
          "with the median poll p50 (all of them in the JSON).  Kernel times by HIP events (`acl_set_timing`) in a pass of their own.",
          f"Both paths gave the same changes at every step: {'yes' if not mism else 'NO (' + str(mism) + ' steps differ)'}.", "",
          f"| W | sets | row bytes | poll p50 us | poll {tail} us | alternative p50 us | alternative {tail} us | of it the lookup p50 us | kernels per poll us | walk us | diff us | changes per step |",
          "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in res["runs"]:
        n = len(r["poll_p50_us"])
        if not n:
            continue
        k = sorted(range(n), key=lambda i: r["poll_p50_us"][i])[n // 2]
        md.append(f"| {r['watchers']} | {r['sets']} | {r['row_bytes']} | {r['poll_p50_us'][k]} | {r['poll_p99_us'][k]} | {r['alt_p50_us'][k]} | {r['alt_p99_us'][k]} | "
                  f"{r['alt_lookup_p50_us'][k]} | {r['kernels_us_per_poll'][k]} | {r['walk_us_per_poll'][k]} | {r['diff_us_per_poll'][k]} | {r['changes_per_step'][k]} |")
    with open(out + ".md", "w") as f:
        f.write("\n".join(md) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c4", choices=["c4", "c5r"])
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--watchers", default="1,64,1024")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--md-from", default="", help="a result .json of an earlier run: write --out.json / --out.md from it again (no GPU needed)")
    a = ap.parse_args()
    if a.md_from:
        write_out(json.load(open(a.md_from)), a.out)
        return 0
    import aclgpu
    from aclgpu import workloads

    w = workloads.c4(scale=a.scale, batch=4096) if a.workload == "c4" else workloads.c5(scale=a.scale, batch=4096)
    res = {"workload": a.workload, "scale": a.scale, "relationships": w.ntuples, "pods": w.nobjects["pod"], "steps": a.steps, "warmup": a.warmup, "repeat": a.repeat, "runs": []}
    rng = np.random.default_rng(7)
    mismatches = 0
    t0 = time.perf_counter()
    with aclgpu.Engine(w.schema, device=0) as e:
        # names for the subjects and the groups the writes name (dense ids follow interning order: name k is id k of the bulk load)
        for k in range(w.nobjects["user"]):
            e.intern("user", f"user-{k}")
        for k in range(w.nobjects["group"]):
            e.intern("group", f"group-{k}")
        w.load(e)
        e.lookup_ids("pod", "view", "user", "", 0)  # forward + reverse snapshot
        res["load_s"] = round(time.perf_counter() - t0, 1)
        words = (e.object_count("pod") + 31) // 32
        for W in [int(x) for x in a.watchers.split(",")]:
            users = np.unique(w.subj)[:W].astype(np.uint32)  # subjects of the request mix: they hold something
            if users.size < W:
                users = np.arange(W, dtype=np.uint32)
            sets, owner = [], []  # (set, [global watcher index]); a refused add opens the next set
            for i, u in enumerate(users.tolist()):
                while True:
                    if not sets:
                        sets.append((e.watch_set("pod", "view", "user"), []))
                    try:
                        sets[-1][0].add(f"user-{u}", from_now=True)
                        sets[-1][1].append(i)
                        break
                    except aclgpu.AclError as ex:
                        if ex.code != aclgpu.ERR_RESOURCE_EXHAUSTED or not sets[-1][1]:
                            raise
                        sets.append((e.watch_set("pod", "view", "user"), []))
            pinned = [e.host_alloc(W * words * 4).view(np.uint32).reshape(W, words) for _ in range(2)]
            counts = np.zeros(W, dtype=np.uint64)

            def poll_all():  # (the timed part: the records as numpy arrays)
                return [(idx, s.poll()[1]) for s, idx in sets]

            def as_tuples(polled):
                return [(idx[int(r["watcher"])], int(r["resource_id"]), int(r["gained"])) for idx, recs in polled for r in recs]

            poll_all()  # baseline (FROM_NOW: nothing reported)
            e.lookup_ids_batch("pod", "view", "user", "", users, out=(pinned[0], counts))
            cur = 0
            live = set()
            run = {"watchers": W, "sets": len(sets), "row_bytes": words * 4, "poll_p50_us": [], "poll_p99_us": [], "alt_p50_us": [], "alt_p99_us": [], "alt_lookup_p50_us": [],
                   "changes_per_step": [], "kernels_us_per_poll": [], "walk_us_per_poll": [], "diff_us_per_poll": []}

            def step_write():
                u, g = int(users[rng.integers(W)]), int(rng.integers(w.nobjects["group"]))
                rel = ("group", f"group-{g}", "member", "user", f"user-{u}", "")
                if live and rng.random() < 0.5:
                    rel = live.pop()
                    e.write([(aclgpu.OP_DELETE, rel)])
                else:
                    live.add(rel)
                    e.write([(aclgpu.OP_TOUCH, rel)])

            for rep in range(a.repeat):
                tp, ta, tl, nch = [], [], [], []
                for step in range(a.warmup + a.steps):
                    step_write()
                    t = time.perf_counter()
                    polled = poll_all()
                    t1 = time.perf_counter()
                    got = as_tuples(polled)
                    nxt = cur ^ 1
                    bms, _c = e.lookup_ids_batch("pod", "view", "user", "", users, out=(pinned[nxt], counts))
                    t2 = time.perf_counter()
                    assert bms is pinned[nxt]  # (written in place: the rows are the pinned ones)
                    x = pinned[cur] ^ pinned[nxt]
                    changed = np.flatnonzero(x.reshape(-1))
                    t3 = time.perf_counter()
                    want = changes_by_xor(x, pinned[nxt], list(range(W)))
                    cur = nxt
                    if got != want:
                        mismatches += 1
                    assert (changed.size == 0) == (not want)
                    if step >= a.warmup:
                        tp.append(t1 - t)
                        ta.append(t3 - t1)
                        tl.append(t2 - t1)
                        nch.append(len(got))
                run["poll_p50_us"].append(pct(tp, 50))
                run["poll_p99_us"].append(pct(tp, 99))
                run["alt_p50_us"].append(pct(ta, 50))
                run["alt_p99_us"].append(pct(ta, 99))
                run["alt_lookup_p50_us"].append(pct(tl, 50))
                run["changes_per_step"].append(round(float(np.mean(nch)), 1))
                # kernel times by HIP events: a pass of its own (polls only)
                e.set_timing(True)
                e.stats_reset()
                for step in range(a.steps):
                    step_write()
                    poll_all()
                st = e.stats()
                e.set_timing(False)
                run["kernels_us_per_poll"].append(round(st["kernel_ms"] * 1e3 / a.steps, 1))
                run["walk_us_per_poll"].append(round((st["rev_local_ms"] + st["expand_ms"]) * 1e3 / a.steps, 1))
                run["diff_us_per_poll"].append(round((st["kernel_ms"] - st["rev_local_ms"] - st["expand_ms"]) * 1e3 / a.steps, 1))
                e.lookup_ids_batch("pod", "view", "user", "", users, out=(pinned[cur], counts))  # (the alternative's baseline follows the untimed writes)
            res["runs"].append(run)
            print(json.dumps(run), flush=True)
            if a.out:
                write_out(dict(res, mismatches=mismatches), a.out)
            for s, _idx in sets:
                s.close()
            for p in pinned:
                e.host_free(p)
    res["mismatches"] = mismatches
    print(json.dumps(res), flush=True)
    if a.out:
        write_out(res, a.out)
    return 0 if mismatches == 0 else 1


if __name__ == "__main__":
    sys.exit(main())

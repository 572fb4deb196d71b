"""Subject-direction watch sets on C4 (scale 1.0): what a poll of W watched pods costs, and what the same answer costs the way a caller gets it without
them.  Modelled on tools/watch_set_bench.py.

Two legs, each on its own engine:
  membership  C4's schema and relationships; one group-membership write per step (a TOUCH or the DELETE of a `group#member@user` relationship: no
              relationship of a pod changes, the reference-shaped watch hears nothing).  pod#view is monotone: a poll is walk + diff.
  bans        C4's relationships under a tool-local schema that adds `relation banned: user` to pod and `- banned` to pod#view, with --bans bans
              written; the write per step is a ban of somebody who holds view on a watched pod, or the unban of an earlier one.  Every candidate of
              every watched pod is confirmed by a Check at every poll: the leg the device confirmation exists for.
Per leg and W in --watchers:
  refresh     the first read after a write patches the snapshot and rebuilds LookupSubjects' subject rows, whichever call it is: an empty
              acl_lookup_subjects_batch (n = 0) right after the step's write pays it here, timed on its own, so that neither column below holds it;
  poll        p50 / max of acl_watch_set_poll;
  kernels     HIP-event time per poll (acl_set_timing, in a pass of its own: event records would otherwise sit inside the timed polls), split into
              walk (acl_stats subj_local_ms: k_subj_local and the copy of its rows into the set's array), confirm (refine_ms + local_ms + expand_ms: candidate records, items, the Check, apply) and diff (the rest);
  alternative acl_lookup_subjects_batch of the W pods into host rows + a numpy XOR against the previous rows, same process, same writes (every step:
              write, poll, alternative).
Both must give the same changes at every step (asserted; a mismatch ends the run with a non-zero status).

  python tools/subject_watch_bench.py --out profiles/subject_watch_c4
writes <out>.json and <out>.md."""
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


def changes_by_xor(prev, cur):
    """the alternative's diff on the host: [k, 3] (row, subject id, gained) ordered by (row, subject id)"""
    x = prev ^ cur
    r, wd = np.nonzero(x)
    if not r.size:
        return np.zeros((0, 3), dtype=np.int64)
    bits = np.unpackbits(np.ascontiguousarray(x[r, wd]).view(np.uint8).reshape(-1, 4), axis=1, bitorder="little")
    k, b = np.nonzero(bits)
    return np.stack([r[k], wd[k].astype(np.int64) * 32 + b, (cur[r, wd][k] >> b.astype(np.uint32)) & 1], axis=1).astype(np.int64)


def schema_with_bans(schema):
    a = schema.index("definition pod")
    pod = schema[a:].replace("relation creator: user", "relation creator: user\n  relation banned: user").replace(
        "permission view = viewer + creator + namespace->view", "permission view = (viewer + creator + namespace->view) - banned")
    assert "banned" in pod and "- banned" in pod
    return schema[:a] + pod


def write_out(res, out):
    with open(out + ".json", "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    mism = res.get("mismatches", 0)
    md = [f"# Subject-direction watch sets on C4 (scale {res['scale']}: {res['relationships']} relationships, {res['users']} users)", "",
          "`tools/subject_watch_bench.py`: one write per step, then the set's poll and -- same process, same writes -- the alternative a caller has",
          "without the set: `acl_lookup_subjects_batch` of the W pods into host rows + a numpy XOR against the previous rows.",
          "The first read after a write patches the snapshot and rebuilds the subject rows whichever call it is: an empty lookup pays that first (refresh).",
          f"{res['steps']} timed steps after {res['warmup']} warm-up steps; the tail column is the maximum of those steps.  Kernel times by HIP events",
          "(`acl_set_timing`) in a pass of their own: walk = `k_subj_local`, confirm = candidate records + items + the Check + apply, diff = the rest.",
          f"Both paths gave the same changes at every step: {'yes' if not mism else 'NO (' + str(mism) + ' steps differ)'}.", "",
          "| leg | W | row bytes | refresh p50 us | poll p50 us | poll max us | alternative p50 us | alternative max us | of it the lookup p50 us | kernels per poll us | walk us | confirm us | diff us | candidates per poll | changes per step |",
          "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in res["runs"]:
        md.append(f"| {r['leg']} | {r['watchers']} | {r['row_bytes']} | {r['refresh_p50_us']} | {r['poll_p50_us']} | {r['poll_max_us']} | {r['alt_p50_us']} | {r['alt_max_us']} | {r['alt_lookup_p50_us']} | "
                  f"{r['kernels_us_per_poll']} | {r['walk_us_per_poll']} | {r['confirm_us_per_poll']} | {r['diff_us_per_poll']} | {r['candidates_per_poll']} | {r['changes_per_step']} |")
    with open(out + ".md", "w") as f:
        f.write("\n".join(md) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--watchers", default="1,64,1024")
    ap.add_argument("--legs", default="membership,bans")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bans", type=int, default=4000)
    ap.add_argument("--out", default="")
    ap.add_argument("--md-from", default="", help="a result .json of an earlier run: write --out.json / --out.md from it again (no GPU needed)")
    a = ap.parse_args()
    if a.md_from:
        write_out(json.load(open(a.md_from)), a.out)
        return 0
    import aclgpu
    from aclgpu import workloads

    w = workloads.c4(scale=a.scale, batch=4096)
    watchers = [int(x) for x in a.watchers.split(",")]
    nwatch = max(watchers)
    res = {"workload": "c4", "scale": a.scale, "relationships": w.ntuples, "users": w.nobjects["user"], "pods": w.nobjects["pod"], "steps": a.steps, "warmup": a.warmup,
           "bans": a.bans, "runs": []}
    rng = np.random.default_rng(7)
    mismatches = 0
    for leg in a.legs.split(","):
        schema = w.schema if leg == "membership" else schema_with_bans(w.schema)
        t0 = time.perf_counter()
        with aclgpu.Engine(schema, device=0) as e:
            # names for what the writes and the sets name (dense ids follow interning order: name k is id k of the bulk load)
            for k in range(w.nobjects["user"]):
                e.intern("user", f"user-{k}")
            for k in range(w.nobjects["group"]):
                e.intern("group", f"group-{k}")
            for k in range(nwatch):
                e.intern("pod", f"pod-{k}")
            w.load(e)
            if leg == "bans":
                pairs = np.unique(np.stack([rng.integers(0, 2 * nwatch, size=a.bans), rng.integers(0, w.nobjects["user"], size=a.bans)], axis=1), axis=0)
                e.add_edges("pod", "banned", "user", "", pairs[:, 0].astype(np.uint32), pairs[:, 1].astype(np.uint32))
            rt, pm, st = e.type_id("pod"), e.relation_id("pod", "view"), e.type_id("user")
            words = (e.object_count("user") + 31) // 32
            print(json.dumps({"leg": leg, "load_s": round(time.perf_counter() - t0, 1)}), flush=True)
            for W in watchers:
                rids = np.arange(W, dtype=np.uint32)
                ws = e.subject_watch_set("pod", "view", "user")
                for k in range(W):
                    ws.add(f"pod-{k}", from_now=True)
                rows = [np.zeros((W, words), dtype=np.uint32) for _ in range(2)]
                counts, flags = np.zeros(W, dtype=np.uint64), np.zeros(W, dtype=np.uint8)

                def alternative(dst):
                    e._check(e._L.acl_lookup_subjects_batch(e._h, rt, pm, st, -1, rids.ctypes.data, W, dst.ctypes.data, words, counts.ctypes.data, flags.ctypes.data, None, None))

                ws.poll()  # baseline (FROM_NOW: nothing reported)
                alternative(rows[0])
                cur, live = 0, []

                def step_write():
                    if live and rng.random() < 0.5:
                        e.write([(aclgpu.OP_DELETE, live.pop(int(rng.integers(len(live)))))])
                        return
                    if leg == "membership":
                        rel = ("group", f"group-{int(rng.integers(w.nobjects['group']))}", "member", "user", f"user-{int(rng.integers(w.nobjects['user']))}", "")
                    else:  # somebody who holds view on a watched pod
                        k = int(rng.integers(W))
                        held = np.flatnonzero(np.unpackbits(rows[cur][k].view(np.uint8), bitorder="little"))
                        u = int(held[rng.integers(held.size)]) if held.size else int(rng.integers(w.nobjects["user"]))
                        rel = ("pod", f"pod-{k}", "banned", "user", f"user-{u}", "")
                    if rel not in live:
                        live.append(rel)
                    e.write([(aclgpu.OP_TOUCH, rel)])

                def refresh():
                    e._check(e._L.acl_lookup_subjects_batch(e._h, rt, pm, st, -1, None, 0, None, words, None, None, None, None))

                tr, tp, ta, tl, nch = [], [], [], [], []
                for step in range(a.warmup + a.steps):
                    step_write()
                    tw = time.perf_counter()
                    refresh()
                    t = time.perf_counter()
                    _rev, recs = ws.poll()
                    t1 = time.perf_counter()
                    nxt = cur ^ 1
                    alternative(rows[nxt])
                    t2 = time.perf_counter()
                    x = rows[cur] ^ rows[nxt]
                    changed = np.flatnonzero(x.reshape(-1))
                    t3 = time.perf_counter()
                    want = changes_by_xor(rows[cur], rows[nxt])
                    got = np.stack([recs["watcher"], recs["resource_id"], recs["gained"]], axis=1).astype(np.int64) if recs.size else np.zeros((0, 3), dtype=np.int64)
                    cur = nxt
                    if not np.array_equal(got, want):
                        mismatches += 1
                    assert (changed.size == 0) == (want.shape[0] == 0)
                    if step >= a.warmup:
                        tr.append(t - tw)
                        tp.append(t1 - t)
                        ta.append(t3 - t1)
                        tl.append(t2 - t1)
                        nch.append(int(got.shape[0]))
                # kernel times by HIP events: a pass of its own (polls only)
                e.set_timing(True)
                e.stats_reset()
                for step in range(a.steps):
                    step_write()
                    ws.poll()
                s = e.stats()
                e.set_timing(False)
                alternative(rows[cur])  # (the bans leg picks its next write from these rows)
                walk, confirm = s["subj_local_ms"], s["refine_ms"] + s["local_ms"] + s["expand_ms"]
                run = {"leg": leg, "watchers": W, "row_bytes": words * 4, "refresh_p50_us": pct(tr, 50), "poll_p50_us": pct(tp, 50), "poll_max_us": pct(tp, 100), "alt_p50_us": pct(ta, 50), "alt_max_us": pct(ta, 100),
                       "alt_lookup_p50_us": pct(tl, 50), "changes_per_step": round(float(np.mean(nch)), 1), "kernels_us_per_poll": round(s["kernel_ms"] * 1e3 / a.steps, 1),
                       "walk_us_per_poll": round(walk * 1e3 / a.steps, 1), "confirm_us_per_poll": round(confirm * 1e3 / a.steps, 1),
                       "diff_us_per_poll": round((s["kernel_ms"] - walk - confirm) * 1e3 / a.steps, 1), "candidates_per_poll": round(s["check_items"] / a.steps, 1)}
                res["runs"].append(run)
                print(json.dumps(run), flush=True)
                if a.out:
                    write_out(dict(res, mismatches=mismatches), a.out)
                ws.close()
    res["mismatches"] = mismatches
    print(json.dumps(res), flush=True)
    if a.out:
        write_out(res, a.out)
    return 0 if mismatches == 0 else 1


if __name__ == "__main__":
    sys.exit(main())

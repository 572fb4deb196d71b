"""Explain with proofs on C4 (1 M objects, 100 000 users, 5-level nested groups at scale 1.0): profiles/explain_proof_c4.{json,md}.

C4's relationships under a tool-local schema that adds `relation banned: user` to pod and `- banned` to pod#view (the bans leg of
tools/subject_watch_bench.py), with --bans bans on pairs of the workload's own Check stream.  For 1, 64 and 4 096 granted items of that stream:
  acl_explain_proof_bulk_ids   call p50 / p99 after two warm-up calls, and the call's event-timed kernel time (acl_set_timing) minus that of the same Check
                               called on its own: the proof passes (k_proof_rows + k_proof_items + the candidates' Check + k_proof_pick + k_proof_winner)
  acl_check_bulk_ids           of the same items
  acl_explain_bulk_ids         of the same items on the same graph under C4's own, monotone schema (a second engine in the same process)
Every timed answer is compared with Check's; a sample of --sample proofs per size is held to tests/proof_checker.py's rules: every hop is one of the loaded
relationships, every absent goal answers NO by the C oracle loaded with the same graph (the Python oracle does not hold 10 M relationships), and the item
derives from the hops and the absences within 50 dispatches.  No speed bar: the figures are recorded.

  python tools/explain_proof_bench.py --out profiles/explain_proof_c4        (on a box with the GPU; --quick: fewer calls)"""
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


def schema_with_bans(schema):
    a = schema.index("definition pod")
    pod = schema[a:].replace("relation creator: user", "relation creator: user\n  relation banned: user").replace(
        "permission view = viewer + creator + namespace->view", "permission view = (viewer + creator + namespace->view) - banned")
    assert "banned" in pod and "- banned" in pod
    return schema[:a] + pod


class SampleChecker:
    """tests/proof_checker.py's ProofChecker over a graph too large for the Python oracle: S is a predicate, absences are asked of the C oracle alone.
    It knows no tupleset rows, so it is only for schemas that subtract no arrow and hold no `.all()` -- on any other it refuses to judge."""

    def __init__(self, schema, stored, oracle):
        from oracle.pyoracle import NO, parse_schema
        from tests.proof_checker import ProofChecker

        class Stored:
            def __contains__(self, h):
                return stored(h)

        class NoRows(dict):  # (the rules for `- t->p` and `t.all(p)` read EVERY parent of an object: a predicate cannot list them)
            def get(self, *a):
                raise AssertionError("SampleChecker cannot judge a schema that subtracts an arrow or uses .all(): it holds no tupleset rows")

        class Both:  # (the checker asks `py` for NO and `c` for (1, 0): both answers are the C oracle's here)
            def check(self, *a):
                return NO if oracle.check(*a) == (1, 0) else "not NO"

        self.pc = ProofChecker.__new__(ProofChecker)
        self.pc.defs, self.pc.S, self.pc.py, self.pc.c, self.pc.rows = parse_schema(schema), Stored(), Both(), oracle, NoRows()

    def check(self, item, hops, absent):
        self.pc.check(item, hops, absent)


def write_md(res, path):
    out = ["# Explain with proofs on C4 with bans: call time next to Check and Explain", "",
           f"`tools/explain_proof_bench.py` on one MI355X, C4 at scale {res['scale']} ({res['relationships']} relationships) under `pod#view = (viewer + creator +",
           f"namespace->view) - banned` with {res['bans']} bans on pairs of the Check stream; granted items of that stream.  One process; `proof passes` is the",
           "call's event-timed kernel time (`acl_set_timing`) minus that of the same Check called on its own -- rows, items, the candidates' Check, pick and",
           "winner together, and the walks of the monotone stretches (`k_explain_local`; `DESIGN.md` 15).  `Explain` is `acl_explain_bulk_ids` of the same items on",
           "the same graph under C4's own monotone schema.  The other columns are host wall-clock times of whole calls.", "",
           "| items | proof p50 us | proof p99 us | proof passes us (mean) | candidate Check passes per call | Check p50 us | Explain (monotone schema) p50 us | hops / absences per proof (mean) |",
           "|---|---|---|---|---|---|---|---|"]
    for n, c in res["calls"].items():
        out.append(f"| {n} | {c['proof_p50_us']} | {c['proof_p99_us']} | {c['proof_kernel_us']} | {c['launches_per_call']} | {c['check_p50_us']} | {c['explain_p50_us']} | "
                   f"{c['hops_mean']} / {c['absent_mean']} |")
    out += ["", f"First proof call on the snapshot: {res['first_call_ms']} ms (it builds and uploads the subject rows).",
            f"Answers compared with Check: {res['answers_compared']}, mismatches: {res['mismatches']}; proofs held to the checker: {res['proofs_checked']}, "
            f"refused: {res['proofs_refused']}; region overflow retries: {res['overflow_retries']}.", ""]
    with open(path, "w") as f:
        f.write("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--bans", type=int, default=4000)
    ap.add_argument("--sample", type=int, default=64)
    ap.add_argument("--quick", action="store_true", help="fewer calls")
    ap.add_argument("--out", default="", help="write <out>.json and <out>.md")
    a = ap.parse_args()
    import aclgpu
    from aclgpu import workloads
    from oracle import orc

    t0 = time.perf_counter()
    w = workloads.c4(scale=a.scale, batch=16384)
    schema = schema_with_bans(w.schema)
    rng = np.random.default_rng(7)
    pick = rng.choice(w.res.size, size=min(a.bans, w.res.size), replace=False)
    bans = np.unique(np.stack([w.res[pick], w.subj[pick]], axis=1), axis=0).astype(np.uint32)
    res = {"workload": "C4 + bans", "scale": a.scale, "relationships": int(w.ntuples + bans.shape[0]), "bans": int(bans.shape[0]), "calls": {}}
    edges = {}
    for ert, rel, est, srel, r, s in w.edges:
        edges.setdefault((ert, rel, est, srel), set()).update(((r.astype(np.uint64) << np.uint64(32)) | s.astype(np.uint64)).tolist())
    edges[("pod", "banned", "user", "")] = set(((bans[:, 0].astype(np.uint64) << np.uint64(32)) | bans[:, 1].astype(np.uint64)).tolist())
    stored = lambda h: ((int(h[1]) << 32) | int(h[4])) in edges.get((h[0], h[2], h[3], h[5]), ())  # noqa: E731
    o = orc.Oracle(schema)
    w.load(o)
    o.add_edges("pod", "banned", "user", "", bans[:, 0], bans[:, 1])
    checker = SampleChecker(schema, stored, o)
    with aclgpu.Engine(schema, device=0) as e, aclgpu.Engine(w.schema, device=0) as mono:
        w.load(e)
        e.add_edges("pod", "banned", "user", "", bans[:, 0], bans[:, 1])
        w.load(mono)
        stream = e.make_items("pod", "view", w.res, "user", "", w.subj)
        perm, err = e.check_bulk_ids(stream)  # (builds the forward snapshot)
        items = stream[(perm == aclgpu.PERM_HAS) & (err == 0)][:4096]
        mitems = mono.make_items("pod", "view", items["resource_id"], "user", "", items["subject_id"])
        mono.explain_ids(mitems[:1])
        res["load_s"] = round(time.perf_counter() - t0, 2)
        t = time.perf_counter()
        e.explain_proof_ids(items[:1])
        res["first_call_ms"] = round((time.perf_counter() - t) * 1e3, 2)
        r0 = e.stats()["overflow_retries"]
        e.set_timing(True)
        tname = {e.type_id(tn): tn for tn in ("user", "group", "namespace", "pod")}
        rname = {(e.type_id(tn), e.relation_id(tn, m)): m for tn, ms in (("group", ["member"]), ("namespace", ["viewer", "creator", "view"]),
                                                                        ("pod", ["namespace", "viewer", "creator", "banned", "view"])) for m in ms}

        def hop_tuples(raw):
            return [(tname[int(h["rtype"])], str(int(h["rid"])), rname[(int(h["rtype"]), int(h["relation"]))], tname[int(h["stype"])], str(int(h["sid"])),
                     "" if int(h["srel"]) == 0xFFFF else rname[(int(h["stype"]), int(h["srel"]))]) for h in raw]

        def absent_tuples(raw):
            return [(tname[int(x["resource_type"])], str(int(x["resource_id"])), rname[(int(x["resource_type"]), int(x["permission"]))], tname[int(x["subject_type"])],
                     str(int(x["subject_id"])), "") for x in raw]

        mism = compared = checked = refused = 0
        for n in [k for k in (1, 64, 4096) if k <= items.size]:
            reps = (3 if a.quick else (max(30, a.sample) if n == 1 else 30)) if n < 4096 else (2 if a.quick else 8)
            xs, cs, ms, km, launches, hop_n, abs_n = [], [], [], [], [], [], []
            sampled = 0
            for k in range(reps + 2):
                sl = slice(0, n) if n > 1 else slice(k % items.size, k % items.size + 1)
                it = items[sl]
                s0 = e.stats()
                t = time.perf_counter()
                p, er, fl, off, hops, aoff, absent = e.explain_proof_ids(it)
                xs.append(time.perf_counter() - t)
                s1 = e.stats()
                t = time.perf_counter()
                cp, ce = e.check_bulk_ids(it)
                cs.append(time.perf_counter() - t)
                s2 = e.stats()
                t = time.perf_counter()
                mono.explain_ids(mitems[sl])
                ms.append(time.perf_counter() - t)
                km.append((s1["kernel_ms"] - s0["kernel_ms"]) - (s2["kernel_ms"] - s1["kernel_ms"]))
                launches.append((s1["check_passes"] - s0["check_passes"]) - (s2["check_passes"] - s1["check_passes"]))  # the candidates' Check passes
                compared += it.size
                mism += int((p != cp).sum() + (er != ce).sum() + (fl != aclgpu.EXPLAIN_PROOF).sum())
                hop_n += np.diff(off.astype(np.int64)).tolist()
                abs_n += np.diff(aoff.astype(np.int64)).tolist()
                for i in range(it.size):
                    if sampled >= a.sample:
                        break
                    if n == 1 and k < 2:
                        continue
                    sampled += 1
                    checked += 1
                    item = ("pod", str(int(it["resource_id"][i])), "view", "user", str(int(it["subject_id"][i])), "")
                    try:
                        checker.check(item, hop_tuples(hops[off[i]:off[i + 1]]), absent_tuples(absent[aoff[i]:aoff[i + 1]]))
                    except AssertionError as ex:
                        refused += 1
                        print("REFUSED", item, str(ex)[:300], file=sys.stderr)
            res["calls"][str(n)] = {"proof_p50_us": pct(xs[2:], 50), "proof_p99_us": pct(xs[2:], 99), "proof_kernel_us": round(float(np.mean(km[2:])) * 1e3, 1),
                                    "launches_per_call": round(float(np.mean(launches[2:])), 1), "check_p50_us": pct(cs[2:], 50), "explain_p50_us": pct(ms[2:], 50),
                                    "hops_mean": round(float(np.mean(hop_n)), 2), "absent_mean": round(float(np.mean(abs_n)), 2), "proofs_sampled": sampled}
        res["answers_compared"], res["mismatches"], res["proofs_checked"], res["proofs_refused"] = compared, mism, checked, refused
        res["overflow_retries"] = int(e.stats()["overflow_retries"] - r0)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out + ".json", "w") as f:
            f.write(line + "\n")
        write_md(res, a.out + ".md")
    return 0 if mism == 0 and refused == 0 else 1


if __name__ == "__main__":
    sys.exit(main())

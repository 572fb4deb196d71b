"""Child process of tests/test_hashed_rows_{cpu,gpu}.py: run with ACL_SEEDED_ROWS=0 (latched once per process, plan.cpp seeded_rows), where
EVERY hashed row is two-choice.  Builds the graphs with ACL_DEBUG_ROWS=1 and prints one JSON line: what ran and the row reports' totals.
  --cpu   store-only builds of reduced C2 / C4 and the bans graph (no GPU)
  (none)  the same graphs on the GPU against the oracle -- C2 and C4 Check + LookupResources, the bans graph in the walk and the level
          loop -- and a short tools/fuzz_gpu.py run per schema (c4, combine: writes, so the patcher places two-choice rows too)
Exit 0 only when every answer equals the oracle's."""
import importlib.util
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "spicedb-kubeapi-proxy_amd")]
os.environ["ACL_DEBUG_ROWS"] = "1"

import numpy as np  # noqa: E402

import aclgpu  # noqa: E402
from aclgpu import workloads  # noqa: E402
from oracle import orc  # noqa: E402
from tests import hashed_rows_graph as H  # noqa: E402
from tests.test_combine_gpu import SCHEMA_BANS, bans_graph  # noqa: E402


def same(a, b, what):
    if not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])):
        raise AssertionError(f"{what}: {int((a[0] != b[0]).sum())} permissionships and {int((a[1] != b[1]).sum())} error codes differ from the oracle")


def graphs():
    c2 = workloads.c2(scale=0.05, batch=20000)
    c4 = workloads.c4(scale=0.02, batch=30000, n_user=20000)
    E, n = bans_graph(11)
    return c2, c4, (E, n)


def run_cpu(done):
    c2, c4, (E, _n) = graphs()
    for w in (c2, c4):
        e = aclgpu.Engine(w.schema, store_only=True)
        w.load(e)
        e.selfcheck_snapshot()
        e.close()
        done.append(f"build {w.name}")
    e = aclgpu.Engine(SCHEMA_BANS, store_only=True)
    H.load(e, E)
    e.selfcheck_snapshot()
    e.close()
    done.append("build bans")


def run_gpu(done):
    c2, c4, (E, n) = graphs()
    for w in (c2, c4):
        o = orc.Oracle(w.schema)
        w.load(o)
        o.freeze()
        rt, perm, st = w.check
        with aclgpu.Engine(w.schema, device=0) as e:
            w.load(e)
            same(e.check_bulk_ids(e.make_items(rt, perm, w.res, st, "", w.subj)), o.check_bulk_ids_mt(8, rt, perm, w.res, st, "", w.subj), f"{w.name} Check")
            for s in np.unique(w.subj)[:4]:
                got = e.lookup_ids(rt, perm, st, "", int(s))
                want = np.sort(np.asarray(o.lookup_ids(rt, perm, st, "", int(s)), dtype=np.uint32))
                if not np.array_equal(got, want):
                    raise AssertionError(f"{w.name} LookupResources of subject {int(s)}: {got.size} ids, the oracle {want.size}")
        done.append(f"{w.name} check+lookup")
    co = orc.Oracle(SCHEMA_BANS)
    H.load(co, E)
    co.freeze()
    rng = np.random.default_rng(3)
    res = rng.integers(0, n["pod"], size=40000).astype(np.uint32)
    sub = rng.integers(0, n["user"], size=40000).astype(np.uint32)
    for mode in ("walk", "level-loop"):
        if mode == "level-loop":
            os.environ["ACL_LOCAL_MAX"] = "0"  # (read at acl_open)
        with aclgpu.Engine(SCHEMA_BANS, device=0) as e:
            H.load(e, E)
            for perm in ("view", "strict", "loose"):
                same(e.check_bulk_ids(e.make_items("pod", perm, res, "user", "", sub)), co.check_bulk_ids_mt(8, "pod", perm, res, "user", "", sub), f"bans {mode} {perm}")
            st = e.stats()
            if mode == "walk" and not (st["local_passes"] >= 3 and st["expand_launches"] == 0):
                raise AssertionError(f"bans walk: {st['local_passes']} walk passes, {st['expand_launches']} level-loop launches")
            if mode == "level-loop" and not (st["local_passes"] == 0 and st["expand_launches"] > 0):
                raise AssertionError(f"bans level loop: {st['local_passes']} walk passes, {st['expand_launches']} level-loop launches")
        done.append(f"bans {mode}")
    os.environ.pop("ACL_LOCAL_MAX", None)
    spec = importlib.util.spec_from_file_location("fuzz_gpu", os.path.join(ROOT, "tools", "fuzz_gpu.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    for seed, schema in ((41, "c4"), (42, "combine")):
        st = fz.run(seed, 60, verbose=False, schema=schema)  # (asserts every answer itself)
        if not (st["writes"] > 5 and st["snapshot_patches"] >= 1):
            raise AssertionError(f"fuzz {schema}: {st['writes']} writes, {st['snapshot_patches']} patches")
        done.append(f"fuzz {schema}")


def main():
    cpu = "--cpu" in sys.argv[1:]
    done = []
    log = tempfile.TemporaryFile(mode="w+b")
    saved = os.dup(2)
    os.dup2(log.fileno(), 2)  # the row reports are written to fd 2 by the library
    try:
        (run_cpu if cpu else run_gpu)(done)
    finally:
        sys.stderr.flush()
        os.dup2(saved, 2)
        log.seek(0)
        text = log.read().decode(errors="replace")
        sys.stderr.write(text)
    reps = H.parse_reports(text)
    print(json.dumps(dict(seeded_rows=os.environ.get("ACL_SEEDED_ROWS"), done=done,
                          reports=[dict(rows=r["rows"], two=r["two"], slow=r["slow"], largest=r["largest"]) for r in reps])))


if __name__ == "__main__":
    main()

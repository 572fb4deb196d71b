"""The cases of the read campaign (tools/fuzz_gpu.py run_reads) and the coverage conditions both test files hold their stats to:
tests/test_fuzz_reads_cpu.py runs every case as an oracle-only dry run, tests/test_fuzz_reads_gpu.py with the engine.

A seed whose stream does not exercise what its case is for fails the conditions on a CPU, before the case is run on a GPU."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# id -> (seed, steps, run_reads keywords)
CASES = {
    "c4-cyclic": (31, 140, dict()),
    "c4-recycle-compactions": (37, 140, dict(recycle=True, compact_early=True)),
    "combine-acyclic": (33, 120, dict(schema="combine", acyclic=True)),
    "combine-acyclic-recycle-compactions": (34, 100, dict(schema="combine", acyclic=True, recycle=True, compact_early=True)),
    "combine-cyclic-depth": (35, 60, dict(schema="combine", depth_case=True, read_share=0.9)),
    # the schemas' expiring variants under a moving clock (fuzz_gpu.Clock); on the cyclic C4 graphs a smaller probe batch, and in the first fewer steps, for
    # the oracle's time.  The recycle / compactions case keeps its twin's 140 steps: nestings that run out drop the two-hop rows, the garbage they leave makes
    # the engine rebuild or adopt a background build every few steps, and at 80 steps only 19 or 20 of its snapshot changes were patches in place.
    "c4-expiring": (62, 80, dict(expiring=True, probe=100)),
    "c4-expiring-recycle-compactions": (77, 140, dict(expiring=True, recycle=True, compact_early=True, probe=100)),
    "combine-acyclic-expiring": (82, 120, dict(schema="combine", acyclic=True, expiring=True)),
}


def load_fuzz():
    spec = importlib.util.spec_from_file_location("fuzz_gpu", os.path.join(ROOT, "tools", "fuzz_gpu.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    return fz


def run_case(case, engine):
    seed, steps, kw = CASES[case]
    return load_fuzz().run_reads(seed, steps, engine=engine, verbose=False, **kw)


def kinds_of(case):
    kw = CASES[case][2]
    if kw.get("depth_case"):
        return ["subjects", "multi"]
    return ["subjects", "explain", "denial", "multi", "cursors", "revoke"] + (["proof"] if kw.get("schema") == "combine" else []) + (["watch"] if kw.get("expiring") else [])


def assert_oracle_side_coverage(case, st):
    """what the stream itself decides: the same figures in a dry run and in a run with the engine (the run asserts every answer; these say it had something to assert)"""
    kw = CASES[case][2]
    for k in kinds_of(case):
        assert st["rounds_" + k] >= 3, (k, st)
    assert st["skipped"] * 10 <= st["rounds"], st
    assert st["writes_accepted"] >= 20, st  # (a read follows most of them: the engine's own count is snapshot_patches)
    if kw.get("depth_case"):  # four LookupSubjects targets in all, picked so that both outcomes occur
        assert st["subj_rows"] <= 4 and st["subj_depth"] >= 1 and st["subj_rows"] - st["subj_depth"] >= 1, st
        return
    assert st["subj_nonempty"] * 10 >= st["subj_rows"] * 6 and st["subj_empty"] >= 1 and st["subj_interned_only"] >= 1, st
    assert st["subj_depth"] == 0, st  # (the acyclic cases and the C4 cases: no LookupSubjects call ends at the depth limit)
    if kw.get("recycle"):
        assert st["subj_first_seen"] >= 1, st
    assert st["witnesses"] >= 200 and st["replayed"] >= 64, st
    if kw.get("schema") == "combine":
        assert st["proofs"] >= 30, st
    else:
        assert st["denied_with_grants"] >= 20, st
    assert st["cursors_read_later"] >= 4 and st["derives"] >= 1 and st["cursors_closed"] >= 1 and st["cursors_left_open"] >= 1, st
    assert st["revoke_with_cuts"] >= 20 and st["revoke_items"] > st["revoke_with_cuts"], st  # (granted items with a single delete that revokes them, and some with none)
    if kw.get("expiring"):
        from tests.fuzz_clock import assert_clock_coverage
        assert_clock_coverage(st, kw.get("schema") == "combine")
        assert st["cursors_read_after_clock_move"] >= 2, st  # (a cursor keeps the rows of its open across an expiry)
        # a poll per direction whose expected difference holds a loss, behind a clock move with no accepted write in between
        assert st["watch_polls"] >= 3 and st["watch_loss_behind_clock_res"] >= 1 and st["watch_loss_behind_clock_sub"] >= 1, st


def assert_engine_side_coverage(case, st):
    """what only the engine can say: how its snapshot followed the writes under the reads"""
    kw = CASES[case][2]
    assert st["snapshot_patches"] >= 20, st
    if kw.get("recycle"):
        assert st["ids_recycled"] >= 5 and st["cursors_read_after_recycling"] >= 1, st
    if kw.get("compact_early"):
        assert st["snapshot_compactions"] >= 1 and st["cursors_read_after_compaction"] >= 1, st

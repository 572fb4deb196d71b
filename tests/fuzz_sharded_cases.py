"""The cases of the sharded campaign (tools/fuzz_gpu.py run_sharded) and the coverage conditions both test files hold their stats to:
tests/test_fuzz_sharded_cpu.py runs every case dry (the oracles' script, then its writes on one store-only engine per rank whose patched host snapshot is
verified against the store at every read step), tests/test_fuzz_sharded_gpu.py replays the script on the logical shards of one GPU.

Shard placements (fnv1a(type) mod world, tests/shard_double.py fnv1a; the dry run reads the same off acl_shard_of_type):
  world 2: pod 0, group + namespace 1            world 5: pod + group 4, namespace 3            world 8: pod 4, group 1, namespace 3
  world 3: pod, group AND namespace all on rank 0 (user on 2) -- nothing would cross a shard, so the second recycle case runs at
  world 4: pod 0, group 1, namespace 3 (user 3; rank 2 owns nothing).

What a case cannot show, by the oracles' own definitions (expected values come from them alone):
  * on the C4 schema (no `-`, `&`, .all()) a LookupResources never fails -- the oracle fails a lookup only for a candidate that the positive relaxation grants and
    the full schema errs on, and the two are one schema there -- and LookupSubjects leaves a subject beyond the depth limit out silently.  The cyclic C4 cases are
    therefore held to "no lookup and no LookupSubjects call fails" and to the Check conditions; failing lookups and LookupSubjects calls are the cyclic combine case's.
  * the cyclic combine case asks three LookupSubjects targets in all, one a round, by turns one that must fail and one that must answer (the contract's Python
    oracles need over a second per target there, as in the read campaign's depth case), and one namespace's viewer relation, the answered call there that crosses
    shards: the conditions on the share of non-empty rows, on empty and interned-only rows and on wildcard rows are the other cases'.

The `*-expiring-*` cases run the schemas' expiring variants under a moving clock (fuzz_gpu.Clock): a clock move is a script step that every rank applies to its
own engine before the next read, followed by the clock's probe batch as a Check step; the dry run verifies every rank's patched snapshot behind every move.

A seed whose stream does not exercise what its case is for fails the conditions on a CPU, before the case is replayed on a GPU."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# id -> (seed, steps, world, run_sharded keywords)
CASES = {
    "c4-cyclic-w2": (31, 100, 2, dict(exchange="allgather")),
    "c4-recycle-compactions-w5": (39, 100, 5, dict(recycle=True, compact_early=True, exchange="alltoall")),
    "c4-cyclic-w8-xcap8": (31, 80, 8, dict(exchange="alltoall", xcap=8)),
    "combine-acyclic-w8": (33, 100, 8, dict(schema="combine", acyclic=True)),
    "combine-acyclic-recycle-compactions-w4": (43, 100, 4, dict(schema="combine", acyclic=True, recycle=True, compact_early=True)),
    "combine-cyclic-depth-w5": (35, 60, 5, dict(schema="combine", depth_case=True, read_share=0.9)),
    # the schemas' expiring variants under a moving clock (fuzz_gpu.Clock): a clock step is a script step every rank applies to its own engine
    "c4-expiring-w5": (98, 60, 5, dict(expiring=True, exchange="alltoall", probe=60)),  # (60 steps, a probe batch of 60: the oracle's time on the cyclic graph)
    "combine-acyclic-expiring-w8": (93, 100, 8, dict(schema="combine", acyclic=True, expiring=True)),
}
# the cases whose stream outruns the LookupSubjects loop's burst hint too (a native call whose levels exceed 2 and the call's before it)
SUBJECTS_HINT_OUTRUN = ("c4-cyclic-w2", "c4-recycle-compactions-w5", "c4-cyclic-w8-xcap8", "combine-acyclic-w8", "combine-acyclic-recycle-compactions-w4")

ERR_FAILED_PRECONDITION = 9  # include/aclgpu.h ACL_ERR_FAILED_PRECONDITION: what ShardCall::begin answers the step protocol on a schema with `-` / `&` / .all()


def load_fuzz():
    spec = importlib.util.spec_from_file_location("fuzz_gpu", os.path.join(ROOT, "tools", "fuzz_gpu.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    return fz


def run_case(case, engine):
    seed, steps, world, kw = CASES[case]
    return load_fuzz().run_sharded(seed, steps, world, engine=engine, verbose=False, **kw)


def assert_oracle_side_coverage(case, st):
    """what the stream itself decides: the same figures in a dry run and in a replay (the replay records every wrong answer; these say it had something to answer)"""
    kw = CASES[case][3]
    combine, cyclic = kw.get("schema") == "combine", not kw.get("acyclic")
    assert st["writes_accepted"] >= 20 and st["writes_read_before_next"] * 3 >= st["writes_accepted"] * 2, st
    for k in ("check", "lookup", "subjects"):
        assert st["rounds_" + k] >= 3, (k, st)
    assert st["skipped"] * 10 <= st["rounds"], st
    if kw.get("depth_case"):
        assert st["subj_rows"] <= 4 and st["subj_answered_over_arrow"] >= 1, st  # (... and an answered call whose walk crosses shards)
    else:
        assert st["subj_nonempty"] * 10 >= st["subj_rows"] * 6 and st["subj_empty"] >= 1 and st["subj_interned_only"] >= 1, st
        if combine:
            assert st["subj_wildcard_excluded"] >= 1, st
    if kw.get("recycle"):
        assert st["subj_first_seen"] >= 1 and st["check_first_seen_items"] >= 1, st
    if cyclic:
        assert st["check_depth_items"] >= 1 and st["check_outruns_expected"] >= 1, st  # (a batch with an item at the depth limit behind a batch without one)
    else:
        assert st["check_depth_items"] == 0, st
    if cyclic and combine:
        assert st["lookup_calls_failed"] >= 1 and st["lookup_rows_nonempty"] >= 1 and st["subj_calls_failed"] >= 1 and st["subj_calls_answered"] >= 1, st
    else:  # (see the header: nothing fails on a monotone schema, and nothing ends at the depth limit without cycles)
        assert st["lookup_calls_failed"] == 0 and st["subj_calls_failed"] == 0 and st["subj_depth"] == 0, st
    if kw.get("expiring"):
        from tests.fuzz_clock import assert_clock_coverage
        assert_clock_coverage(st, combine)
        for k in ("check", "lookup", "subjects"):  # a read round of each loop behind a clock move with no accepted write in between
            assert st["reads_behind_clock_" + k] >= 1, (k, st)


def assert_cpu_engine_side_coverage(case, st):
    """the dry run's store-only shard engines: every selfcheck passed (it raises otherwise); on every rank that owns a relationship-bearing type at least ten
    reads found the snapshot patched in place and one found it rebuilt, or adopted from a background build with the writes since replayed"""
    world, kw = CASES[case][2], CASES[case][3]
    assert len(st["dry_ranks"]) == world and sorted(t for r in st["dry_ranks"] for t in r["owns"]) == ["group", "namespace", "pod"], st["dry_ranks"]
    assert len([r for r in st["dry_ranks"] if r["owns"]]) >= 2, st["dry_ranks"]
    for r in st["dry_ranks"]:
        if r["owns"]:
            assert r[1] >= 10 and r[0] + r["adopted"] >= 1, r
        if kw.get("recycle"):
            assert r["ids_recycled"] >= 5, r


def assert_gpu_side_coverage(case, st):
    """what only the replay can say: how every rank's snapshot followed the writes, what crossed the shards, where a loop outran its burst or grew and redid"""
    world, kw = CASES[case][2], CASES[case][3]
    combine, cyclic = kw.get("schema") == "combine", not kw.get("acyclic")
    assert len(st["ranks"]) == world and st["calls_equal_on_every_rank"], st["ranks"]
    for r in st["ranks"]:
        if r["owns"]:
            assert r["snapshot_patches"] >= 10, r
            if kw.get("compact_early"):
                assert r["snapshot_compactions"] >= 1, r
        if kw.get("recycle"):
            assert r["ids_recycled"] >= 5, r
        want = [("check", ERR_FAILED_PRECONDITION), ("lookup", ERR_FAILED_PRECONDITION)] if combine else []
        assert sorted(r["refusals"]) == want, r
    calls = st["calls"]  # (step, kind, follows a write, levels, retries, entries_exchanged, host_syncs, export_capacity, behind a clock move)
    if kw.get("expiring"):  # a native call of each loop behind a clock move with no write in between: the rank's snapshot followed the clock alone
        for kind in ("check", "lookup", "subjects"):
            assert any(c[1] == kind and c[8] and not c[2] for c in calls), (kind, "no native call behind a clock move")
    for kind in ("check", "lookup", "subjects"):
        assert sum(c[5] for c in calls if c[1] == kind) > 0, (kind, "no entry crossed a shard")
    if kw.get("xcap"):
        # Retries alone say nothing about the knob (a cyclic Check batch redoes to merge duplicates, a level planned without entries redoes too): the call has to end
        # with a larger export block than the native call before it.  The three loops size their blocks from one capacity per engine and report it alike, so
        # that is growth on this call.  (Before the first call a block holds max(8, xcap) entries.)
        caps = [max(8, kw["xcap"])] + [c[7] for c in calls]
        grew = [c for before, c in zip(caps, calls) if c[4] >= 1 and c[7] > before]
        assert any(c[2] for c in grew), ("no native call behind a write outgrew its export block and redid", grew)
    for loop, wanted in (("check", cyclic), ("subjects", case in SUBJECTS_HINT_OUTRUN)):
        lv = [c[3] for c in calls if c[1].startswith(loop)]
        if wanted:
            assert any(b > 2 and b > a for a, b in zip(lv, lv[1:])), (loop, "no call outran the burst sized by the call before it", lv)

"""A short run of tools/fuzz_gpu.py as a regression test: the engine and the CPU oracle mutate the same nested-group / arrow graph step by step
(write batches with every update kind, filter deletes) and answer the same Check batches (1 ... 70 000 items), single checks through the
micro-batcher and LookupResources requests in between -- every answer, error code and id set equal.  `combine-schema`: the same on the C4 schema
extended with exclusions, intersections, wildcards and a non-monotone userset subject (fuzz_gpu.SCHEMA_COMBINE; VERDICT r3 next #2 "incl. a fuzz
campaign").  The long campaigns are run by hand
(tools/fuzz_gpu.py --seed S --steps N [--burst B --universe U]); profiles/r03_fuzz.txt holds this round's.
`expiring-*`: the schemas' expiring variants (fuzz_gpu.SCHEMA_C4_EXPIRING / SCHEMA_COMBINE_EXPIRING) under a clock that moves forwards and back between the
writes (fuzz_gpu.Clock): a nesting, an arrow's tupleset, a wildcard or a ban runs out -- or comes back -- with no write at all, and a probe batch of 200 Check
items is held to the oracle behind every move.  The seeds are the ones whose oracle-only stream (tools/fuzz_gpu.py --expiring --dry) meets
tests/fuzz_clock.py; profiles/fuzz_expiry.md holds the figures."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
@pytest.mark.parametrize("seed,kw", [(11, {}), (12, dict(burst=300, universe=3)), (13, dict(compact_early=True)), (21, dict(schema="combine")),
                                     (22, dict(schema="combine", compact_early=True)), (23, dict(recycle=True)), (24, dict(recycle=True, schema="combine", compact_early=True)),
                                     (52, dict(expiring=True, probe=80)), (54, dict(expiring=True, schema="combine", compact_early=True)),
                                     (53, dict(expiring=True, acyclic=True, recycle=True))],
                         ids=["small-universe", "write-bursts", "compactions", "combine-schema", "combine-schema-compactions", "recycled-ids", "recycled-ids-combine-compactions",
                              "expiring-c4", "expiring-combine-compactions", "expiring-acyclic-recycle"])
def test_differential_fuzz(seed, kw, aclgpu_lib):
    spec = importlib.util.spec_from_file_location("fuzz_gpu", os.path.join(ROOT, "tools", "fuzz_gpu.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    st = fz.run(seed, 60 if "burst" in kw else (250 if kw else 120), verbose=False, **kw)  # (the oracle's brute-force lookups are what takes the time: ~10 s and ~20 s)
    assert st["writes"] > 5 and st["checks"] > 100 and st["lookups"] >= 1 and st["snapshot_patches"] >= 1  # (the run itself asserts every answer)
    if kw.get("recycle"):
        assert st["ids_recycled"] >= 5  # never-seen names took over the ids of objects that had lost their last relationship, under the reads
    if kw.get("compact_early"):
        assert st["snapshot_compactions"] >= 1  # background builds were adopted in mid-stream, the writes since their start replayed onto them
    if kw.get("expiring"):
        from tests.fuzz_clock import assert_clock_coverage
        assert_clock_coverage(st, kw.get("schema") == "combine")
        if kw.get("acyclic"):
            assert st["keep_route_calls"] >= 1  # (one-user calls took the reverse route, on rows that follow the clock)


@pytest.mark.gpu
def test_differential_fuzz_expiring_keys(aclgpu_lib):
    """The reference's bootstrap schema under the dual write's shapes (lock CREATE behind MUST_NOT_MATCH, lock DELETE, expiring idempotency keys:
    workflow.go:392-462, activity.go:81-102) with a clock that moves seconds to days per step: checks on live / expired / unwritten keys, locks and
    payloads and the read-back of the expiring class equal the oracle's after every step."""
    spec = importlib.util.spec_from_file_location("fuzz_gpu", os.path.join(ROOT, "tools", "fuzz_gpu.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    st = fz.run_expiry(14, 400, verbose=False)
    assert st["writes"] > 100 and st["write_errors"] > 5 and st["clock_moves"] > 20 and st["snapshot_patches"] > 20

"""tools/fuzz_gpu.py run_reads as a regression test: the engine and the CPU oracles mutate the same nested-group / arrow graph step by step (write batches with
every update kind, filter deletes; recycled object ids and adopted background compactions in the cases named for them), and between the writes the engine's
other read paths answer on the snapshot patched in place -- each held to the oracles:
  a. LookupSubjects, batched (1, 5, 33 resources, one with no relationships, under recycling one first named by this stream), the n = 1 call, the string form
     and a group#member subject form: the C oracle's Check on the C4 schema, the contract of tests/subjects_contract.py on the combine schema;
  b. Explain witness: perm / err of the oracle's Check, a witness for every item a monotone permission grants, every witness through tests/explain_checker.py;
  c. Explain proof (combine schema): every granted item proved, the proofs through tests/proof_checker.py;
  d. Explain denial (monotone permissions): the grants through tests/denial_checker.py;
  e. multi-target LookupResources over every relation and permission of the schema, bit for bit the single-target rows and by name the oracle's, its failures
     as include/aclgpu.h states them, and access_review;
  f. lookup, subject and mixed cursors held open across later writes, compactions and recycled ids: the ids stay what they were at every page size, names are
     answered or refused, derived cursors and counts equal the set algebra of the remembered ids; some cursors are left for the engine to close.
  g. Explain for revocation: the cut set of granted monotone items equals the brute force (one relationship out, every item asked, back) and goes through
     tests/revoke_checker.py;
  h. the `*-expiring` cases: the schemas' expiring variants under a clock that moves forwards and back between the writes (fuzz_gpu.Clock) -- a probe batch of
     Check items behind every move, every kind above at the current clock with the hops' expiries in the checkers' replays, cursors read across clock moves,
     and a resource-direction and a subject-direction watch set polled against the difference of the oracle's rows (tests/watch_records.py).
tests/fuzz_reads_cases.py holds the cases and the coverage conditions; tests/test_fuzz_reads_cpu.py runs the same cases without an engine.
The second test is the expiring-keys campaign (run_expiry), which now also asks LookupSubjects and Explain about live and expired idempotency keys."""
import pytest

from tests import fuzz_reads_cases as F

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(F.CASES))
def test_reads_under_writes(case, aclgpu_lib):
    st = F.run_case(case, engine=True)  # (the run itself asserts every answer; one engine, closed at the end with cursors still open)
    print(case, st)
    F.assert_oracle_side_coverage(case, st)
    F.assert_engine_side_coverage(case, st)


def test_reads_on_expiring_keys(aclgpu_lib):
    st = F.load_fuzz().run_expiry(15, 200, verbose=False)
    assert st["writes"] > 50 and st["clock_moves"] > 10 and st["snapshot_patches"] > 10
    assert st["subject_lookups"] >= 300 and st["subject_rows_nonempty"] >= 50 and st["live_keys_explained"] >= 50 and st["expired_keys_explained"] >= 50, st

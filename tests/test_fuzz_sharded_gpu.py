"""tools/fuzz_gpu.py run_sharded as a regression test: the loops of the type-hash sharded graph under a live write stream.  The oracles alone turn the read
campaign's kind of stream (write batches with every update kind, filter deletes; recycled object ids and background compactions in the cases named for them)
into a script of writes and reads with their expected outcomes; every one of 2 to 8 logical shards of one GPU -- one engine per rank over a replicated store,
one thread each -- replays it, and every rank is held to every answer, by name:
  a. Check batches of 1, 7, 64, 900 and 3000 items through acl_shard_check_bulk and, on the same step, through the host-driven step protocol (all-gather or
     all-to-all), the two routes against each other;
  b. LookupResources of 1 and 4 subjects through acl_shard_lookup_bulk and the host-driven protocol; where the oracle fails the lookup every rank raises its code,
     and the next call on that engine answers;
  c. LookupSubjects of 1, 5 and 33 resources with the excluded rows through acl_shard_subjects_bulk (a resource only interned, one without relationships, under
     recycling one first named by the stream; user and group#member subjects), or ACL_ERR_DEPTH on every rank;
  d. write outcomes, filter-delete counts and the ids every rank gives the names it interns.
The host-driven protocol refuses the combine schema (ShardCall::begin): there the native loops alone answer, and the refusal's code is asserted.
tests/fuzz_sharded_cases.py holds the cases and the coverage conditions; tests/test_fuzz_sharded_cpu.py runs the same scripts without a GPU."""
import pytest

from tests import fuzz_sharded_cases as F

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(F.CASES))
def test_sharded_reads_under_writes(case, aclgpu_lib):
    st = F.run_case(case, engine=True)  # (raises with the first record when a rank recorded a wrong answer)
    print(case, {k: v for k, v in st.items() if k != "calls"})
    print(case, "calls", st["calls"])
    F.assert_oracle_side_coverage(case, st)
    F.assert_gpu_side_coverage(case, st)

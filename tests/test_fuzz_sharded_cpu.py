"""The sharded campaign's cases (tests/fuzz_sharded_cases.py) as dry runs of tools/fuzz_gpu.py run_sharded: the oracles' script -- the same writes, reads and
expected values tests/test_fuzz_sharded_gpu.py replays -- and the script's writes on one store-only engine per rank (acl_shard_configure), whose host snapshot,
patched for the types the rank owns, is verified against the store at every read step.  No GPU.  A seed whose stream does not exercise what its case is for
-- too few rounds of a read kind, no Check item at the depth limit in a cyclic case, no failing lookup on the cyclic combine graph, no recycled id, a rank
whose snapshot was never patched under the reads -- fails here."""
import pytest

from tests import fuzz_sharded_cases as F


@pytest.mark.parametrize("case", list(F.CASES))
def test_dry_run_covers_what_the_case_is_for(case):
    st = F.run_case(case, engine=False)
    print(case, st)
    F.assert_oracle_side_coverage(case, st)
    F.assert_cpu_engine_side_coverage(case, st)

"""The read campaign's cases (tests/fuzz_reads_cases.py) as oracle-only dry runs of tools/fuzz_gpu.py run_reads: the same write stream and the same expected
values as tests/test_fuzz_reads_gpu.py computes, no engine and no GPU.  A seed whose stream does not exercise what its case is for -- too few rounds of a
read kind, no empty LookupSubjects row, a LookupSubjects call that ends at the depth limit where none may, too few witnesses, proofs, denied items with
grants or cursors read after later writes -- fails here."""
import pytest

from tests import fuzz_reads_cases as F


@pytest.mark.parametrize("case", list(F.CASES))
def test_dry_run_covers_what_the_case_is_for(case):
    st = F.run_case(case, engine=False)
    print(case, st)
    F.assert_oracle_side_coverage(case, st)

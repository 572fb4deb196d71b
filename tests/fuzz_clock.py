"""The coverage conditions of the expiring cases of tools/fuzz_gpu.py (the Check campaign, the read campaign, the sharded campaign): what a stream with a moving
clock (fuzz_gpu.Clock) must have met for its case to say anything.  They are counted on the oracle side -- the probe batch's answers and the oracle's read
difference across every clock move -- so a dry run decides them, on a CPU, before the case is run on a GPU."""


def assert_clock_coverage(st, combine):
    assert st["clock_forward"] >= 10 and st["clock_back"] >= 3, st
    assert st["lost_by_clock"] >= 10 and st["gained_by_clock_back"] >= 1, st  # (probe answers lost to an expiry; brought back by a clock set back, no write)
    assert st["expired_nestings"] >= 3 and st["expired_tuplesets"] >= 3, st   # (group#member@group#member and pod#namespace relationships that ran out)
    assert st["collected_due"] >= 5, st                                       # (expired for 24 h at an accepted write: the store collects them inside it)
    if combine:
        assert st["expired_bans"] >= 1 and st["gained_by_clock"] >= 1, st     # (a ban's expiry GRANTS: a probe answer gained by a forward move)

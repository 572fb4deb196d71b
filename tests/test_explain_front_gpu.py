"""The three forms of Explain over ONE mixed batch: acl_explain_bulk_ids, acl_explain_proof_bulk_ids and acl_explain_denial_bulk_ids share their call front,
their Check and the classification of its answers (engine_explain.cpp explain_front / check_ids_chunked / explain_classify), so one batch whose neighbours
all fall into different classes must come back from the three with the same perm / err -- acl_check_bulk_ids' and both oracles' -- and with exactly the
flags each form owes each class.  What the records say is held to the three checkers the forms' own suites use."""
import numpy as np
import pytest

from tests import denial_checker as D
from tests import explain_checker as X
from tests import proof_checker as P
from tests.test_explain_denial_gpu import ids_of, named
from tests.test_explain_proof_gpu import Names

pytestmark = pytest.mark.gpu

PERM_NO, PERM_HAS = 1, 2

SCHEMA = """
definition user {}
definition group {
  relation member: user | group#member
}
definition doc {
  relation viewer: user | group#member
  relation banned: user
  permission view = viewer - banned
  permission read = viewer
}
"""
RELS = [("doc", "d", "viewer", "user", "a", ""), ("doc", "d", "viewer", "user", "b", ""), ("doc", "d", "banned", "user", "b", ""),
        ("doc", "d", "viewer", "group", "g", "member"), ("group", "g", "member", "group", "h", "member"), ("group", "h", "member", "user", "c", ""),
        ("doc", "e", "viewer", "user", "a", ""),
        # a relation that nests through a cycle of two groups: a Check that enters it and does not find its subject runs into the depth limit
        ("doc", "loop", "viewer", "group", "x", "member"), ("group", "x", "member", "group", "y", "member"), ("group", "y", "member", "group", "x", "member"),
        ("group", "x", "member", "user", "f", "")]
GRANTED_MONO, GRANTED_NONMONO, DENIED_MONO, DENIED_NONMONO, ERRING = range(5)
BATCH = [(("doc", "d", "read", "user", "c", ""), GRANTED_MONO),
         (("doc", "d", "view", "user", "a", ""), GRANTED_NONMONO),
         (("doc", "e", "read", "user", "c", ""), DENIED_MONO),
         (("doc", "d", "view", "user", "b", ""), DENIED_NONMONO),
         (("doc", "loop", "read", "user", "c", ""), ERRING),
         (("doc", "d", "read", "user", "nobody", ""), DENIED_MONO),  # a subject id no relationship names
         (("doc", "d", "read", "user", "c", ""), GRANTED_MONO),       # two repeats
         (("doc", "d", "view", "user", "b", ""), DENIED_NONMONO)]
ITEMS = [it for it, _ in BATCH]
CLASSES = [cl for _, cl in BATCH]


@pytest.fixture(scope="module")
def aclgpu(aclgpu_lib):
    import aclgpu as m
    return m


@pytest.fixture(scope="module")
def orcs():
    return D.Oracles(SCHEMA, RELS)


@pytest.fixture(scope="module")
def answers(aclgpu):
    """the batch through Check and the three forms, once: (ids, check, explain, proof, denial, the same three with n = 0, names)"""
    with aclgpu.Engine(SCHEMA, device=0) as e:
        e.touch(*RELS)
        ids = ids_of(e, ITEMS)
        got = dict(ids=ids, check=e.check_bulk_ids(ids), explain=e.explain_ids(ids), proof=e.explain_proof_ids(ids), denial=e.explain_denial_ids(ids),
                   empty=[e.explain_ids(ids[:0]), e.explain_proof_ids(ids[:0]), e.explain_denial_ids(ids[:0])])
        nm = Names(e, SCHEMA)
        x, p, d = got["explain"], got["proof"], got["denial"]
        got["witnesses"] = [nm.hops(x[4][x[3][i]:x[3][i + 1]]) for i in range(len(ITEMS))]
        got["proofs"] = [(nm.hops(p[4][p[3][i]:p[3][i + 1]]), nm.absent(p[6][p[5][i]:p[5][i + 1]])) for i in range(len(ITEMS))]
        got["grants"] = [named(e, SCHEMA, ITEMS[i], d[4][d[3][i]:d[3][i + 1]]) for i in range(len(ITEMS))]
    return got


def test_no_two_neighbours_share_a_class():
    assert all(a != b for a, b in zip(CLASSES, CLASSES[1:])) and set(CLASSES) == set(range(5))


def test_perm_and_err_are_checks_and_both_oracles(aclgpu, answers, orcs):
    cperm, cerr = answers["check"]
    for form in ("explain", "proof", "denial"):
        perm, err = answers[form][:2]
        print(form, perm.tolist(), err.tolist())
        assert np.array_equal(perm, cperm) and np.array_equal(err, cerr), form
    for i, (item, cl) in enumerate(BATCH):
        (operm, oerr), y = orcs.check(item)
        print(item, (int(cperm[i]), int(cerr[i])), (operm, oerr), y)
        if cl == ERRING:
            assert oerr == D.orc.ERR_DEPTH and y == "ERR" and int(cerr[i]) == aclgpu.ERR_DEPTH
        else:
            want = PERM_HAS if cl in (GRANTED_MONO, GRANTED_NONMONO) else PERM_NO
            assert (operm, oerr, y) == (want, 0, "HAS" if want == PERM_HAS else "NO")
            assert (int(cperm[i]), int(cerr[i])) == (want, 0)


def test_flags_are_exactly_each_forms_own(aclgpu, answers):
    W, U, PR, DN = aclgpu.EXPLAIN_WITNESS, aclgpu.EXPLAIN_UNSUPPORTED, aclgpu.EXPLAIN_PROOF, aclgpu.EXPLAIN_DENIAL
    table = {GRANTED_MONO: (W, W, 0), GRANTED_NONMONO: (U, PR, 0), DENIED_MONO: (0, 0, DN), DENIED_NONMONO: (0, 0, U), ERRING: (0, 0, 0)}
    for k, form in enumerate(("explain", "proof", "denial")):
        print(form, answers[form][2].tolist())
        assert answers[form][2].tolist() == [table[cl][k] for cl in CLASSES], form


def test_offsets_start_at_zero_never_fall_and_end_at_the_records(answers):
    x, p, d = answers["explain"], answers["proof"], answers["denial"]
    for off, recs in ((x[3], x[4]), (p[3], p[4]), (p[5], p[6]), (d[3], d[4])):
        assert off.size == len(ITEMS) + 1 and off[0] == 0 and np.all(np.diff(off.astype(np.int64)) >= 0) and int(off[-1]) == recs.size
    # an item has records only where its flag says so
    for i, cl in enumerate(CLASSES):
        assert (x[3][i + 1] > x[3][i]) == (cl == GRANTED_MONO)
        assert (p[3][i + 1] > p[3][i]) == (cl in (GRANTED_MONO, GRANTED_NONMONO))
        assert p[5][i + 1] == p[5][i] or cl == GRANTED_NONMONO
        assert d[3][i + 1] == d[3][i] or cl == DENIED_MONO


def test_witnesses_proofs_and_grants_pass_their_checkers(answers, orcs):
    for i, (item, cl) in enumerate(BATCH):
        hops, absent = answers["proofs"][i]
        if cl == GRANTED_MONO:
            X.check_witness(SCHEMA, set(RELS), item, answers["witnesses"][i])
            assert (hops, absent) == (answers["witnesses"][i], [])  # a monotone item's proof is its witness
        if cl in (GRANTED_MONO, GRANTED_NONMONO):
            P.check_proof(SCHEMA, RELS, item, hops, absent)
        if cl == DENIED_MONO:
            assert answers["grants"][i]
            D.check_grants(orcs, item, answers["grants"][i])
    assert answers["witnesses"][0] == answers["witnesses"][6] and answers["grants"][3] == answers["grants"][7] == []  # the repeats


def test_an_empty_batch_is_ok_and_empty(answers):
    for got in answers["empty"]:
        assert all(a.size == 0 for a in got[:3])
        for off, recs in zip(got[3::2], got[4::2]):
            assert off.tolist() == [0] and recs.size == 0

"""Explain proofs without a GPU: the two entry points exist and bind as the header declares them, the new constants are what a C99 compiler sees, a
store-only engine refuses to evaluate, and the proof checker the GPU tests rely on (tests/proof_checker.py) accepts true proofs and refuses broken ones."""
import os
import re
import subprocess

import pytest

from tests import proof_checker as P

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "aclgpu.h")


@pytest.fixture(scope="module")
def aclgpu(aclgpu_lib):
    import aclgpu as m
    return m


def _params(name):
    hdr = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", hdr, flags=re.S)
    assert m, name
    return [p for p in m.group(1).split(",") if p.strip()]


def test_symbols_are_exported_and_bound(aclgpu, aclgpu_lib):
    for name, nparams in (("acl_explain_proof_bulk_ids", 11), ("acl_explain_proof", 7)):
        assert name in aclgpu._lib.SYMBOLS and hasattr(aclgpu_lib, name)
        assert len(_params(name)) == nparams
        assert len(getattr(aclgpu_lib, name).argtypes) == nparams, name
    assert hasattr(aclgpu.Engine, "explain_proof_ids") and hasattr(aclgpu.Engine, "explain_proof")


def test_constants_match_a_c99_compiler(aclgpu, tmp_path):
    src = tmp_path / "proof.c"
    src.write_text('#include <stdio.h>\n#include "aclgpu.h"\nint main(void) {\n'
                   '  printf("%u %u %u %zu\\n", ACL_HOP_SEGMENT, ACL_EXPLAIN_PROOF, ACL_PROOF_MAX_RECORDS, sizeof(acl_explain_hop_t));\n  return 0;\n}\n')
    exe = tmp_path / "proof"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert out == [aclgpu.HOP_SEGMENT, aclgpu.EXPLAIN_PROOF, aclgpu.PROOF_MAX_RECORDS, 20] == [2, 4, 65536, 20]
    # the flags of one hop, and of one item, do not overlap
    assert aclgpu.HOP_SEGMENT & aclgpu.HOP_WILDCARD == 0
    assert len({aclgpu.EXPLAIN_WITNESS, aclgpu.EXPLAIN_UNSUPPORTED, aclgpu.EXPLAIN_PROOF}) == 3 and aclgpu.EXPLAIN_PROOF & (aclgpu.EXPLAIN_WITNESS | aclgpu.EXPLAIN_UNSUPPORTED) == 0


def test_store_only_engine_is_unavailable(aclgpu):
    with aclgpu.Engine(BAN, store_only=True) as e:
        e.touch(("doc", "d", "viewer", "user", "a", ""))
        items = e.make_items("doc", "view", [e.find("doc", "d")], "user", "", [e.find("user", "a")])
        for call in (lambda: e.explain_proof_ids(items), lambda: e.explain_proof_ids(items[:0]), lambda: e.explain_proof("doc", "d", "view", "user", "a"),
                     lambda: e.explain_proof("doc", "nobody-wrote-this", "view", "user", "a")):
            with pytest.raises(aclgpu.AclError) as x:
                call()
            assert x.value.code == aclgpu.ERR_UNAVAILABLE
        # argument errors come first, as for Explain
        with pytest.raises(aclgpu.AclError) as x:
            e.explain_proof("doc", "not an id", "view", "user", "a")
        assert x.value.code == aclgpu.ERR_INVALID_ARGUMENT


# ---------------------------------------------------------------- the checker: hand-written proofs
BAN = """
definition user {}
definition doc {
  relation viewer: user
  relation banned: user
  permission view = viewer - banned
}
"""
BAN_RELS = [("doc", "d", "viewer", "user", "a", ""), ("doc", "d", "viewer", "user", "b", ""), ("doc", "d", "banned", "user", "b", "")]
BAN_ITEM = ("doc", "d", "view", "user", "a", "")
BAN_PROOF = ([BAN_RELS[0]], [("doc", "d", "banned", "user", "a", "")])

BOTH = """
definition user {}
definition doc {
  relation a: user
  relation b: user
  permission both = a & b
}
"""
BOTH_RELS = [("doc", "d", "a", "user", "u", ""), ("doc", "d", "b", "user", "u", ""), ("doc", "d", "a", "user", "v", "")]
BOTH_ITEM = ("doc", "d", "both", "user", "u", "")
BOTH_PROOF = (BOTH_RELS[:2], [])

FOLDERS = """
definition user {}
definition folder {
  relation viewer: user
  permission view = viewer
}
definition doc {
  relation owner: user
  relation parent: folder
  permission hidden = owner - parent->view
  permission shared = parent.all(view)
}
"""
HID_RELS = [("doc", "d", "owner", "user", "u", ""), ("doc", "d", "parent", "folder", "f1", ""), ("doc", "d", "parent", "folder", "f2", ""),
            ("folder", "f1", "viewer", "user", "other", "")]
HID_ITEM = ("doc", "d", "hidden", "user", "u", "")
HID_PROOF = (HID_RELS[:3], [("folder", "f1", "view", "user", "u", ""), ("folder", "f2", "view", "user", "u", "")])

ALL_RELS = [("doc", "d", "parent", "folder", "f1", ""), ("folder", "f1", "viewer", "user", "u", ""), ("doc", "d", "parent", "folder", "f2", ""),
            ("folder", "f2", "viewer", "user", "u", ""), ("folder", "f2", "viewer", "user", "other", "")]
ALL_ITEM = ("doc", "d", "shared", "user", "u", "")
ALL_PROOF = (ALL_RELS[:4], [])

CASES = {"ban": (BAN, BAN_RELS, BAN_ITEM, BAN_PROOF), "both": (BOTH, BOTH_RELS, BOTH_ITEM, BOTH_PROOF), "hidden": (FOLDERS, HID_RELS, HID_ITEM, HID_PROOF),
         "all": (FOLDERS, ALL_RELS, ALL_ITEM, ALL_PROOF)}


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_checker_accepts_the_hand_written_proof(name):
    schema, rels, item, (hops, absent) = CASES[name]
    P.check_proof(schema, rels, item, hops, absent)


@pytest.mark.parametrize("name,drop", [(n, k) for n in sorted(CASES) for k in range(len(CASES[n][3][0]))])
def test_the_checker_refuses_a_proof_with_one_hop_dropped(name, drop):
    """(under `owner - parent->view` that includes the tupleset hops: an absence reached through a tupleset has that relationship among the hops)"""
    schema, rels, item, (hops, absent) = CASES[name]
    with pytest.raises(AssertionError):
        P.check_proof(schema, rels, item, hops[:drop] + hops[drop + 1:], absent)


@pytest.mark.parametrize("name,drop", [(n, k) for n in sorted(CASES) for k in range(len(CASES[n][3][1]))])
def test_the_checker_refuses_a_proof_with_one_absence_dropped(name, drop):
    """... which is also "one parent's absence missing under the arrow" for `owner - parent->view`"""
    schema, rels, item, (hops, absent) = CASES[name]
    with pytest.raises(AssertionError):
        P.check_proof(schema, rels, item, hops, absent[:drop] + absent[drop + 1:])


def test_the_checker_refuses_a_hop_that_is_not_stored():
    with pytest.raises(AssertionError, match="not a stored relationship"):
        P.check_proof(BAN, BAN_RELS[1:], BAN_ITEM, *BAN_PROOF)
    with pytest.raises(AssertionError, match="not a stored relationship"):
        P.check_proof(BOTH, BOTH_RELS, BOTH_ITEM, BOTH_PROOF[0] + [("doc", "d", "b", "user", "v", "")], [])


def test_the_checker_refuses_an_absence_whose_check_is_has():
    # b is a viewer and banned: "not banned" is no fact
    with pytest.raises(AssertionError, match="absent goal"):
        P.check_proof(BAN, BAN_RELS, ("doc", "d", "view", "user", "b", ""), [BAN_RELS[1]], [("doc", "d", "banned", "user", "b", "")])
    # ... and an absence about somebody else is none about the item's subject
    with pytest.raises(AssertionError, match="subject"):
        P.check_proof(BAN, BAN_RELS, ("doc", "d", "view", "user", "b", ""), [BAN_RELS[1]], [("doc", "d", "banned", "user", "a", "")])


def test_the_checker_refuses_one_parents_sub_proof_missing_under_all():
    hops, absent = ALL_PROOF
    for missing in (ALL_RELS[3], ALL_RELS[2]):  # the second parent's viewer hop; the tupleset hop that names the second parent
        with pytest.raises(AssertionError):
            P.check_proof(FOLDERS, ALL_RELS, ALL_ITEM, [h for h in hops if h != missing], absent)
    # .all() over no parent at all grants nothing
    with pytest.raises(AssertionError):
        P.check_proof(FOLDERS, [ALL_RELS[1]], ALL_ITEM, [], [])


def test_the_checker_counts_dispatches_as_the_python_oracle_does():
    """a chain of groups through `active = member - banned`: the longest the oracle grants derives, and its proof placed one group deeper does not"""
    from oracle.pyoracle import ERR, HAS, PyOracle
    schema = """
definition user {}
definition group {
  relation member: user | group#active
  relation banned: user
  permission active = member - banned
}
definition doc {
  relation viewer: group#active
  permission view = viewer
}
"""

    def graph(n):
        return ([("doc", "d", "viewer", "group", "g0", "active")] + [("group", f"g{i}", "member", "group", f"g{i + 1}", "active") for i in range(n)] +
                [("group", f"g{n}", "member", "user", "u", "")])

    def answer(n):
        o = PyOracle(schema)
        for r in graph(n):
            o.touch(*r)
        return o.check("doc", "d", "view", "user", "u")

    n = max(k for k in range(10, 40) if answer(k) == HAS)
    assert answer(n + 1) == ERR
    item = ("doc", "d", "view", "user", "u", "")
    absent = lambda k: [("group", f"g{i}", "banned", "user", "u", "") for i in range(k + 1)]  # noqa: E731
    P.check_proof(schema, graph(n), item, graph(n), absent(n))
    with pytest.raises(AssertionError, match="does not derive"):
        P.check_proof(schema, graph(n + 1), item, graph(n + 1), absent(n + 1))

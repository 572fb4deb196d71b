"""Explain without a GPU: the entry points exist and bind as the header declares them, acl_explain_hop_t is laid out as a C99 compiler lays it out, a
store-only engine refuses to evaluate, the per-op side table names the relationships every program op reads, and the witness checker the GPU tests rely
on accepts a true chain and refuses a broken one."""
import ctypes as C
import os
import re
import subprocess

import pytest

from oracle.pyoracle import HAS, NO
from tests import explain_checker as X

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
    for name, nparams in (("acl_explain_bulk_ids", 9), ("acl_explain", 7), ("acl_selfcheck_explain_ops", 4)):
        assert name in aclgpu._lib.SYMBOLS and hasattr(aclgpu_lib, name)
        assert len(_params(name)) == nparams
        assert len(getattr(aclgpu_lib, name).argtypes) == nparams, name


def test_hop_layout_matches_a_c99_compiler(aclgpu, tmp_path):
    ct = aclgpu._lib.ExplainHop
    fields = [f for f, _t in ct._fields_]
    assert fields == ["rtype", "relation", "rid", "stype", "srel", "sid", "flags"]
    src = tmp_path / "hop.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "aclgpu.h"\nint main(void) {\n  printf("%zu", sizeof(acl_explain_hop_t));\n' +
                   "".join(f'  printf(" %zu", offsetof(acl_explain_hop_t, {f}));\n' for f in fields) +
                   '  printf(" %u %u %u\\n", ACL_HOP_WILDCARD, ACL_EXPLAIN_WITNESS, ACL_EXPLAIN_UNSUPPORTED);\n  return 0;\n}\n')
    exe = tmp_path / "hop"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert out[0] == 20 == C.sizeof(ct) == aclgpu.HOP_DTYPE.itemsize
    assert out[1:8] == [getattr(ct, f).offset for f in fields] == [aclgpu.HOP_DTYPE.fields[f][1] for f in fields] == [0, 2, 4, 8, 10, 12, 16]
    assert out[8:] == [aclgpu.HOP_WILDCARD, aclgpu.EXPLAIN_WITNESS, aclgpu.EXPLAIN_UNSUPPORTED] == [1, 1, 2]


def test_side_table_record_layout_matches_a_c99_compiler(aclgpu, tmp_path):
    ct = aclgpu._lib.ExplainOpRec
    fields = [f for f, _t in ct._fields_]
    src = tmp_path / "op.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "aclgpu.h"\nint main(void) {\n  printf("%zu", sizeof(acl_explain_op_t));\n' +
                   "".join(f'  printf(" %zu", offsetof(acl_explain_op_t, {f}));\n' for f in fields) + '  printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "op"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert out[0] == C.sizeof(ct) == aclgpu.engine.EXPLAIN_OP_DTYPE.itemsize
    assert out[1:] == [getattr(ct, f).offset for f in fields] == [aclgpu.engine.EXPLAIN_OP_DTYPE.fields[f][1] for f in fields]


def test_store_only_engine_is_unavailable(aclgpu):
    from aclgpu import workloads
    with aclgpu.Engine(workloads.SCHEMA_C4, store_only=True) as e:
        e.touch(("pod", "p", "creator", "user", "u", ""))
        items = e.make_items("pod", "view", [e.find("pod", "p")], "user", "", [e.find("user", "u")])
        for call in (lambda: e.explain_ids(items), lambda: e.explain_ids(items[:0]), lambda: e.explain("pod", "p", "view", "user", "u"),
                     lambda: e.explain("pod", "nobody-wrote-this", "view", "user", "u")):
            with pytest.raises(aclgpu.AclError) as x:
                call()
            assert x.value.code == aclgpu.ERR_UNAVAILABLE
        # argument errors come first, as for Check
        with pytest.raises(aclgpu.AclError) as x:
            e.explain("pod", "not an id", "view", "user", "u")
        assert x.value.code == aclgpu.ERR_INVALID_ARGUMENT


OP_PROBE, OP_ENUM, OP_REFLEX, OP_PUSH_SAME, OP_PROBE_HASH = 1, 2, 4, 8, 16  # csrc/plan.hpp


def test_side_table_names_the_relation_every_op_reads(aclgpu):
    """C4's schema: pod#view = viewer + creator + namespace->view inlines the computed usersets `viewer` and `creator` -- their ops sit in view's program
    one dispatch level down and read relations other than the state's own -- and follows the arrow through pod#namespace."""
    from aclgpu import workloads
    with aclgpu.Engine(workloads.SCHEMA_C4, store_only=True) as e:
        e.touch(("pod", "p", "namespace", "namespace", "n", ""), ("pod", "p", "viewer", "group", "g", "member"), ("pod", "p", "viewer", "user", "u", ""),
                ("pod", "p", "creator", "user", "u", ""), ("namespace", "n", "viewer", "group", "g", "member"), ("namespace", "n", "creator", "user", "u", ""),
                ("group", "g", "member", "user", "u", ""), ("group", "g", "member", "group", "h", "member"))
        ops = e.selfcheck_explain_ops()
        tid = {t: e.type_id(t) for t in ("user", "group", "namespace", "pod")}
        rel = lambda t, r: e.relation_id(t, r)  # noqa: E731
        # slots number the members of every definition in schema order
        slot, s = {}, 0
        for t, members in (("user", []), ("group", ["member"]), ("namespace", ["viewer", "creator", "view"]), ("pod", ["namespace", "viewer", "creator", "view"])):
            for m in members:
                assert rel(t, m) == members.index(m)
                slot[(t, m)] = s
                s += 1

        def rows(state, reads=True):
            return [(int(o["rtype"]), int(o["relation"]), int(o["stype"]), int(o["srel"]), int(o["dlevel"]), int(o["kind"]))
                    for o in ops if int(o["slot"]) == slot[state] and (int(o["rtype"]) != 0xFFFF) == reads]

        def cls(t, r, st, sr=None):
            return (tid[t], rel(t, r), tid[st], 0xFFFF if sr is None else rel(st, sr))

        # pod#view: every op reads a relation OTHER than `view`; the inlined ones carry dispatch offset 1, the arrow's tupleset offset 0
        got = {(o[:4], o[4]) for o in rows(("pod", "view"))}
        assert got == {(cls("pod", "viewer", "user"), 1), (cls("pod", "viewer", "group", "member"), 1), (cls("pod", "creator", "user"), 1),
                       (cls("pod", "namespace", "namespace"), 0)}
        kinds = {o[:4]: o[5] for o in rows(("pod", "view"))}
        assert kinds[cls("pod", "viewer", "user")] & OP_PROBE_HASH and kinds[cls("pod", "creator", "user")] & OP_PROBE_HASH
        assert kinds[cls("pod", "viewer", "group", "member")] & OP_ENUM and kinds[cls("pod", "namespace", "namespace")] & OP_ENUM
        assert {(o[:4], o[4]) for o in rows(("namespace", "view"))} == {(cls("namespace", "viewer", "user"), 1), (cls("namespace", "viewer", "group", "member"), 1),
                                                                       (cls("namespace", "creator", "user"), 1)}
        # a relation's own program reads its own classes at offset 0
        assert {(o[:4], o[4]) for o in rows(("group", "member"))} == {(cls("group", "member", "user"), 0), (cls("group", "member", "group", "member"), 0)}
        assert {(o[:4], o[4]) for o in rows(("pod", "viewer"))} == {(cls("pod", "viewer", "user"), 0), (cls("pod", "viewer", "group", "member"), 0)}
        # ops that read nothing: the reflexive ones (view's program holds its own and the inlined states')
        none = rows(("pod", "view"), reads=False)
        assert none and all(o[5] & (OP_REFLEX | OP_PUSH_SAME) for o in none)
        # every op of every program is accounted for
        assert all((int(o["rtype"]) != 0xFFFF) == bool(int(o["kind"]) & (OP_PROBE | OP_ENUM | OP_PROBE_HASH)) for o in ops if int(o["slot"]) != 0xFFFFFFFF)


def test_side_table_marks_a_recursive_reference_as_a_rewrite_step(aclgpu):
    schema = """
definition user {}
definition doc {
  relation parent: doc
  relation viewer: user
  permission view = viewer + parent->view
  permission see = view
}
"""
    with aclgpu.Engine(schema, store_only=True) as e:
        e.touch(("doc", "d", "viewer", "user", "u", ""), ("doc", "d", "parent", "doc", "e", ""))
        ops = e.selfcheck_explain_ops()
        t = e.type_id("doc")
        reads = {(int(o["rtype"]), int(o["relation"])) for o in ops if int(o["rtype"]) != 0xFFFF}
        assert reads == {(t, e.relation_id("doc", "parent")), (t, e.relation_id("doc", "viewer"))}
        for o in ops:
            if int(o["kind"]) & OP_PUSH_SAME:
                assert int(o["rtype"]) == 0xFFFF


CHAIN = [("pod", "ns/a", "namespace", "namespace", "ns", ""), ("namespace", "ns", "viewer", "group", "outer", "member"),
         ("group", "outer", "member", "group", "inner", "member"), ("group", "inner", "member", "user", "u", "")]
ITEM = ("pod", "ns/a", "view", "user", "u", "")


def test_the_checker_accepts_the_four_hop_chain():
    from aclgpu import workloads
    p, c = X.replay(workloads.SCHEMA_C4, ITEM, CHAIN)
    assert p == HAS and c == (2, 0)
    X.check_witness(workloads.SCHEMA_C4, set(CHAIN), ITEM, CHAIN)


@pytest.mark.parametrize("drop", range(4))
def test_the_checker_refuses_the_chain_with_a_hop_removed(drop):
    from aclgpu import workloads
    hops = CHAIN[:drop] + CHAIN[drop + 1:]
    p, c = X.replay(workloads.SCHEMA_C4, ITEM, hops)
    assert p == NO and c == (1, 0)
    with pytest.raises(AssertionError):
        X.check_witness(workloads.SCHEMA_C4, set(CHAIN), ITEM, hops)


def test_the_checker_refuses_a_hop_that_is_not_stored_and_a_chain_out_of_order():
    from aclgpu import workloads
    with pytest.raises(AssertionError):
        X.check_witness(workloads.SCHEMA_C4, set(CHAIN[:3]), ITEM, CHAIN)
    with pytest.raises(AssertionError):
        X.check_witness(workloads.SCHEMA_C4, set(CHAIN), ITEM, [CHAIN[0], CHAIN[2], CHAIN[1], CHAIN[3]])

"""Random schemas on the CPU (tests/schema_gen.py): the two oracles arbitrate each other on every Check item and every LookupResources target of every
corpus seed, the host half of the plan compiler (a store-only engine: build, then a patch per write round, each verified by acl_selfcheck_snapshot)
accepts every schema, and the corpus is held to coverage conditions by the C oracle alone -- a generator that drifts into trivial schemas fails here,
not silently on the GPU.  The device half is tests/test_random_schema_gpu.py."""
import re

import pytest

from oracle import orc
from oracle.pyoracle import PyOracle, SchemaError
from tests import schema_gen as G
from tests.outcomes import outcome
from tests.test_oracle_cross import PY2C

from tests.schema_gen import IDS, SMALL, case_of, load_oracles

DEPTH = (orc.PERM_UNSPEC, orc.ERR_DEPTH)
_answers = {}


def c_answers(mode, seed):
    """the C oracle's answer to every item of the seed's initial relationships, computed once for every test of this file"""
    if (mode, seed) not in _answers:
        c = case_of(mode, seed)
        co, _ = load_oracles(c.schema, c.rels, python=False)
        _answers[(mode, seed)] = [co.check(*q) for q in c.items]
    return _answers[(mode, seed)]


@pytest.fixture(scope="module")
def aclgpu(aclgpu_lib):
    import aclgpu as m
    return m


def test_generator_is_deterministic_and_well_formed():
    from oracle.pyoracle import _ID, _REL, _TYPE
    for mode in G.MODES:
        c = G.gen(G.CORPUS[mode][0], mode)
        assert c == G.gen(G.CORPUS[mode][0], mode)
        assert c != G.gen(G.CORPUS[mode][0] + 1, mode)
        assert 3 <= len(c.types) <= 5 and "user" in c.types and c.members.keys() == c.types.keys() - {"user"}
        for t, ms in c.members.items():
            assert _TYPE.match(t) and all(_REL.match(m) and len(m) >= 3 for m in ms), (t, ms)
            assert all(s != "user" and m == "" for s, m in c.allowed[(t, ms[0])]), "the tupleset allows plain objects only"
        assert all(_ID.match(o) for os_ in c.types.values() for o in os_)
        assert len(c.rounds) == 3 and all(d and t for d, t in c.rounds)
        assert not any(G.NOBODY in r for r in G.live_after(c, 3) + c.rels)
        if mode == "wide":
            assert all(len(os_) == 40 for t, os_ in c.types.items() if t != "user") and len(c.users) == 100 and 150 <= len(c.rels) <= 400
        else:
            assert all(len(os_) == 3 for t, os_ in c.types.items() if t != "user") and len(c.users) == 4 and 8 <= len(c.rels) <= 40
            assert len(c.items) == sum(3 * len(ms) for ms in c.members.values()) * 8 and len(c.subjects) == 8
        if mode == "monotone":
            assert not re.search(r"&| - |\.all\(", c.schema)
    assert len(SMALL) == 36 and len(G.CORPUS["wide"]) == 6


@pytest.mark.parametrize("mode,seed", SMALL, ids=IDS)
def test_oracles_agree(mode, seed):
    c = case_of(mode, seed)
    co, po = load_oracles(c.schema, c.rels)
    want = c_answers(mode, seed)
    for q, w in zip(c.items, want):
        assert w == PY2C[po.check(*q)], q
    for t in c.lookup_targets:
        assert outcome(co.lookup, *t) == outcome(po.lookup_resources, *t), t
    assert (orc.PERM_HAS, 0) in want and (orc.PERM_NO, 0) in want, "every seed has a granted and a denied item"


def test_host_compiler_accepts_every_schema_and_patches(aclgpu):
    """no corpus seed is refused (the 30-operand limit included); the snapshot verifies after the load and after each write round"""
    codes = []
    for mode, seed in G.corpus(G.MODES):
        c = case_of(mode, seed)
        with aclgpu.Engine(c.schema, store_only=True) as e:
            e.write([(aclgpu.OP_TOUCH, r) for r in c.rels])
            assert e.selfcheck_snapshot() is False  # the first call builds
            for deletes, touches in c.rounds:
                e.write([(aclgpu.OP_DELETE, r) for r in deletes] + [(aclgpu.OP_TOUCH, r) for r in touches])
                codes.append(e.selfcheck_snapshot_code())  # (verified inside the library: raises on any mismatch)
    assert 1 in codes, "no update of the corpus was a patch"


def test_no_case_holds_a_branching_cycle_through_a_combining_permission():
    """the generator's structural rule (schema_gen.branching_cycle), on the graphs tests/test_combine_gpu.py pins the engine's contract with: the
    teams that nest through `active` in a simple cycle are within it, the ones that nest in two ways are not, groups that nest in two ways under
    `-` are (their cycle runs through a relation); and every corpus case obeys it after the load and after every write round"""
    from oracle.pyoracle import parse_schema
    defs = parse_schema("""
definition user {}
definition group {
  relation member: user | group#member
  relation banned: user
  permission active = member - banned
}
definition team {
  relation member: user | team#active
  relation banned: user
  permission active = member - banned
}""")
    simple = [orc.parse_rel(t) for t in ("team:t0#member@team:t1#active", "team:t1#member@team:t0#active", "team:t1#member@user:deep")]
    branching = [orc.parse_rel(t) for t in ("team:b0#member@team:b0#active", "team:b0#member@team:b1#active", "team:b1#member@team:b0#active")]
    groups = [orc.parse_rel(t) for t in ("group:g0#member@group:g0#member", "group:g0#member@group:g1#member", "group:g1#member@group:g0#member")]
    assert G.branching_cycle(defs, simple) is None and G.branching_cycle(defs, groups) is None
    assert G.branching_cycle(defs, simple + branching + groups) == ("team", "b0", "member")
    assert G.branching_cycle(defs, groups, monotone_too=True) == ("group", "g0", "member")
    assert G.branching_cycle(parse_schema("definition user {}\ndefinition doc {\n relation viewer: user\n permission view = (view & viewer) + (view - viewer)\n}"), (), [("doc", "x")])
    assert G.branching_cycle(parse_schema("definition user {}\ndefinition doc {\n relation viewer: user\n permission view = (view - viewer) + viewer\n}"), (), [("doc", "x")]) is None
    for mode, seed in G.corpus(G.MODES):
        c = case_of(mode, seed)
        defs = parse_schema(c.schema)
        for n in range(4):
            assert G.branching_cycle(defs, G.live_after(c, n)) is None, (mode, seed, n)


def _perm_lines(schema):
    return re.findall(r"definition (\w+) \{(.*?)\}", schema, flags=re.S)


def test_corpus_coverage():
    nm = [(m, s) for m, s in SMALL if m != "monotone"]
    assert sum(DEPTH in c_answers(m, s) for m, s in nm) * 2 >= len(nm), "depth errors"
    for what in ("&", " - ", ".all(", ".any(", ":*"):
        assert sum(what in case_of(m, s).schema for m, s in nm) * 4 >= len(nm), what
    onto_permission = [any(x in G.PERM_NAMES for fs in case_of(m, s).allowed.values() for _, x in fs) for m, s in nm]
    assert sum(onto_permission) * 4 >= len(nm), "usersets onto permissions"
    # a granted item of a monotone seed whose permission is arrows and nothing else: the grant came through an arrow
    through_arrow = 0
    for seed in G.CORPUS["monotone"]:
        c = case_of("monotone", seed)
        only_arrows = set()
        for t, body in _perm_lines(c.schema):
            for p, expr in re.findall(r"permission (\w+) = (.*)", body):
                leaves = [x for x in re.split(r"[\s()+]+", expr) if x and x != "nil"]
                if leaves and all("->" in x or ".any" in x for x in leaves):
                    only_arrows.add((t, p))
        through_arrow += any(w == (orc.PERM_HAS, 0) and (q[0], q[2]) in only_arrows for q, w in zip(c.items, c_answers("monotone", seed)))
    assert through_arrow >= 1


REFUSED = {
    "an arrow over a relation that allows T:*": """
definition user {}
definition doc {
  relation parent: doc | doc:*
  relation viewer: user
  permission view = viewer + parent->view
}""",
    ".all(m) over a subject type without m": """
definition user {}
definition folder { relation viewer: user }
definition org { relation owner: user }
definition doc {
  relation parent: folder | org
  permission view = parent.all(viewer)
}""",
    "an unknown reference": """
definition user {}
definition doc {
  relation viewer: user
  permission view = viewer + editor
}""",
    "a caveat": """
caveat on_weekdays(day int) { day < 6 }
definition user {}
definition doc {
  relation viewer: user
  permission view = viewer
}""",
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_refusals_agree(what, aclgpu):
    schema = REFUSED[what]
    with pytest.raises(orc.OracleError):
        orc.Oracle(schema)
    with pytest.raises(SchemaError):
        PyOracle(schema)
    with pytest.raises(aclgpu.AclError):
        aclgpu.Engine(schema, store_only=True)


def test_operand_limit_is_the_engines_alone(aclgpu):
    """plan.hpp kMaxLeaves: 31 operands under `&` are refused by the engine, by its own message, and taken by both oracles; 30 are taken by all three"""
    def schema(n):
        rels = "\n".join(f"  relation rel{i:02d}: user" for i in range(n))
        return "definition user {}\ndefinition doc {\n" + rels + "\n  permission view = " + " & ".join(f"rel{i:02d}" for i in range(n)) + "\n}\n"
    for n in (30, 31):
        orc.Oracle(schema(n))
        PyOracle(schema(n))
    aclgpu.Engine(schema(30), store_only=True).close()
    with pytest.raises(aclgpu.AclError) as ei:
        aclgpu.Engine(schema(31), store_only=True)
    assert "combines more than 30 operands" in str(ei.value)

"""Explain proofs on the GPU (engine_proof.cpp; k_explain_local for the monotone stretches, k_proof_rows / _items / _pick / _winner) through the C ABI's Python mirror.

acl_explain_proof_bulk_ids = Check + a proof: perm / err are acl_check_bulk_ids' for the same items; a granted item on a monotone permission comes back as
acl_explain_bulk_ids returns it, a granted item on a permission with `-`, `&` or `.all()` beneath comes with hops and absences.  Every returned proof goes
through ONE checker (tests/proof_checker.py): the hops are stored, every absent goal answers NO by both oracles on the full set, and the item derives from
the hops and the absences within 50 dispatches."""
import random

import numpy as np
import pytest

from oracle import orc
from oracle.pyoracle import ERR, HAS, NO, PyOracle, parse_schema
from tests import explain_checker as X
from tests import proof_checker as P

pytestmark = pytest.mark.gpu

PERM_NO, PERM_HAS = 1, 2


@pytest.fixture(scope="module")
def aclgpu(aclgpu_lib):
    import aclgpu as m
    return m


class Names:
    """acl_explain_hop_t / acl_item_t records -> (rtype, rid, rel, stype, sid, srel) tuples; named=False: objects loaded by id, spelled as decimal ids"""

    def __init__(self, e, schema, named=True):
        defs = parse_schema(schema)
        self.tname = {e.type_id(t): t for t in defs}
        self.rname = {(e.type_id(t), e.relation_id(t, m)): m for t, d in defs.items() for m in d.members}
        self.obj = (lambda t, i: e.object_name(t, i)) if named else (lambda t, i: str(i))

    def hops(self, raw):
        out = []
        for h in raw:
            rt, st = self.tname[int(h["rtype"])], self.tname[int(h["stype"])]
            sid = "*" if int(h["flags"]) & 1 else self.obj(st, int(h["sid"]))
            srel = "" if int(h["srel"]) == 0xFFFF else self.rname[(int(h["stype"]), int(h["srel"]))]
            out.append((rt, self.obj(rt, int(h["rid"])), self.rname[(int(h["rtype"]), int(h["relation"]))], st, sid, srel))
        return out

    def absent(self, raw):
        out = []
        for a in raw:
            rt, st = self.tname[int(a["resource_type"])], self.tname[int(a["subject_type"])]
            srel = "" if int(a["subject_relation"]) == 0xFFFF else self.rname[(int(a["subject_type"]), int(a["subject_relation"]))]
            out.append((rt, self.obj(rt, int(a["resource_id"])), self.rname[(int(a["resource_type"]), int(a["permission"]))], st, self.obj(st, int(a["subject_id"])), srel))
        return out


def item_ids(e, item):
    """a named item as one acl_item_t (every name known to the engine)"""
    rt, rid, perm, st, sid, srel = item
    return e.make_items(rt, perm, [e.find(rt, rid)], st, srel, [e.find(st, sid)])


def segments_ok(aclgpu, raw):
    """ACL_HOP_SEGMENT sits exactly on the hops that do not continue the hop before them"""
    for k in range(len(raw)):
        starts = k > 0 and ((int(raw[k]["rtype"]), int(raw[k]["rid"])) != (int(raw[k - 1]["stype"]), int(raw[k - 1]["sid"])) or bool(int(raw[k - 1]["flags"]) & aclgpu.HOP_WILDCARD))
        assert bool(int(raw[k]["flags"]) & aclgpu.HOP_SEGMENT) == starts, (k, raw)


def prove(aclgpu, e, schema, rels, item):
    """one named item through BOTH entry points: they agree with each other and with Check, and a proof passes the checker.
    Returns (perm, err, flags, hops as tuples, absences as tuples)."""
    from aclgpu.text import parse_relationship
    p, er, fl, lines = e.explain_proof(*item)
    assert (p, er) == e.check(*item)
    perm, err, flags, off, raw, aoff, araw = e.explain_proof_ids(item_ids(e, item))
    assert (int(perm[0]), int(err[0]), int(flags[0])) == (p, er, fl)
    assert off.tolist() == [0, len(raw)] and aoff.tolist() == [0, len(araw)]
    nm = Names(e, schema)
    hops, absent = nm.hops(raw), nm.absent(araw)
    assert [parse_relationship(ln) for ln in lines if not ln.startswith("not ")] == hops
    assert [parse_relationship(ln[4:]) for ln in lines if ln.startswith("not ")] == absent
    assert lines == [ln for ln in lines if not ln.startswith("not ")] + [ln for ln in lines if ln.startswith("not ")]  # the hops first
    assert fl in (0, aclgpu.EXPLAIN_WITNESS, aclgpu.EXPLAIN_PROOF)
    if fl:
        assert p == PERM_HAS and er == 0
        P.check_proof(schema, rels, item, hops, absent)
        segments_ok(aclgpu, raw)
    else:
        assert hops == [] and absent == []
    if fl == aclgpu.EXPLAIN_WITNESS:
        assert absent == []
        X.check_witness(schema, set(rels), item, hops)
    return p, er, fl, hops, absent


# ---------------------------------------------------------------- 1. the batch Explain answers and flags, now proved
BAN = """
definition user {}
definition doc {
  relation viewer: user
  relation banned: user
  relation editor: user
  permission view = viewer - banned
  permission edit = editor
}
"""


def test_the_items_explain_flags_unsupported_are_proved(aclgpu):
    rels = [("doc", "d", "viewer", "user", "a", ""), ("doc", "d", "viewer", "user", "b", ""), ("doc", "d", "banned", "user", "b", ""), ("doc", "d", "editor", "user", "a", "")]
    named = [("doc", "d", "view", "user", "a", ""), ("doc", "d", "edit", "user", "a", ""), ("doc", "d", "view", "user", "b", ""), ("doc", "d", "edit", "user", "b", ""),
             ("doc", "d", "view", "user", "a", ""), ("doc", "d", "edit", "user", "a", "")]
    with aclgpu.Engine(BAN, device=0) as e:
        e.touch(*rels)
        items = np.concatenate([item_ids(e, it) for it in named])
        perm, err, flags, off, raw, aoff, araw = e.explain_proof_ids(items)
        cperm, cerr = e.check_bulk_ids(items)
        assert np.array_equal(perm, cperm) and np.array_equal(err, cerr)
        assert perm.tolist() == [PERM_HAS, PERM_HAS, PERM_NO, PERM_NO, PERM_HAS, PERM_HAS] and not err.any()
        assert flags.tolist() == [aclgpu.EXPLAIN_PROOF, aclgpu.EXPLAIN_WITNESS, 0, 0, aclgpu.EXPLAIN_PROOF, aclgpu.EXPLAIN_WITNESS]
        assert off.tolist() == [0, 1, 2, 2, 2, 3, 4] and aoff.tolist() == [0, 1, 1, 1, 1, 2, 2]
        nm = Names(e, BAN)
        for i in (0, 4):
            assert nm.hops(raw[off[i]:off[i + 1]]) == [rels[0]] and nm.absent(araw[aoff[i]:aoff[i + 1]]) == [("doc", "d", "banned", "user", "a", "")]
            P.check_proof(BAN, rels, named[i], [rels[0]], nm.absent(araw[aoff[i]:aoff[i + 1]]))
        # the monotone items: byte for byte what Explain returns; and Explain itself still flags, not proves
        xperm, xerr, xflags, xoff, xraw = e.explain_ids(items)
        assert xflags.tolist() == [aclgpu.EXPLAIN_UNSUPPORTED, aclgpu.EXPLAIN_WITNESS, 0, 0, aclgpu.EXPLAIN_UNSUPPORTED, aclgpu.EXPLAIN_WITNESS]
        for i in (1, 5):
            assert raw[off[i]:off[i + 1]].tobytes() == xraw[xoff[i]:xoff[i + 1]].tobytes() and xoff[i + 1] - xoff[i] == 1
        p, er, fl, lines = e.explain_proof(*named[0])
        assert (p, er, fl) == (PERM_HAS, 0, aclgpu.EXPLAIN_PROOF) and lines == ["doc:d#viewer@user:a", "not doc:d#banned@user:a"]
        assert e.explain_proof(*named[1]) == e.explain(*named[1])  # a monotone item: the text of acl_explain
        assert e.explain_proof(*named[2]) == (PERM_NO, 0, 0, [])


# ---------------------------------------------------------------- 2. hand graphs, the proof pinned where it is unique
def test_intersection_needs_both_hops(aclgpu):
    schema = """
definition user {}
definition doc {
  relation a: user
  relation b: user
  permission both = a & b
}
"""
    rels = [("doc", "d", "a", "user", "u", ""), ("doc", "d", "b", "user", "u", ""), ("doc", "d", "a", "user", "v", "")]
    with aclgpu.Engine(schema, device=0) as e:
        e.touch(*rels)
        p, er, fl, hops, absent = prove(aclgpu, e, schema, rels, ("doc", "d", "both", "user", "u", ""))
        assert (p, er, fl) == (PERM_HAS, 0, aclgpu.EXPLAIN_PROOF) and hops == rels[:2] and absent == []
        assert prove(aclgpu, e, schema, rels, ("doc", "d", "both", "user", "v", "")) == (PERM_NO, 0, 0, [], [])


def test_arrow_into_an_exclusion_behind_two_nested_groups(aclgpu):
    schema = """
definition user {}
definition group {
  relation member: user | group#member
}
definition namespace {
  relation viewer: user | group#member
  relation banned: user
  permission view = viewer - banned
}
definition pod {
  relation namespace: namespace
  permission view = namespace->view
}
"""
    chain = [("pod", "p", "namespace", "namespace", "ns", ""), ("namespace", "ns", "viewer", "group", "outer", "member"),
             ("group", "outer", "member", "group", "inner", "member"), ("group", "inner", "member", "user", "u", "")]
    rels = chain + [("group", "inner", "member", "user", "w", ""), ("namespace", "ns", "banned", "user", "w", ""), ("namespace", "ns", "viewer", "user", "other", "")]
    with aclgpu.Engine(schema, device=0) as e:
        e.touch(*rels)
        p, er, fl, hops, absent = prove(aclgpu, e, schema, rels, ("pod", "p", "view", "user", "u", ""))
        assert (p, er, fl) == (PERM_HAS, 0, aclgpu.EXPLAIN_PROOF) and hops == chain and absent == [("namespace", "ns", "banned", "user", "u", "")]
        assert prove(aclgpu, e, schema, rels, ("pod", "p", "view", "user", "w", "")) == (PERM_NO, 0, 0, [], [])
        # the group's own membership is monotone: a witness, as Explain gives it
        p, er, fl, hops, absent = prove(aclgpu, e, schema, rels, ("group", "outer", "member", "user", "u", ""))
        assert fl == aclgpu.EXPLAIN_WITNESS and hops == chain[2:]


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


@pytest.mark.parametrize("nparents", [0, 1, 3])
def test_exclusion_of_an_arrow_gives_an_absence_and_a_tupleset_hop_per_parent(aclgpu, nparents):
    owner = ("doc", "d", "owner", "user", "u", "")
    parents = [("doc", "d", "parent", "folder", f"f{k}", "") for k in range(nparents)]
    rels = [owner] + parents + [("folder", f"f{k}", "viewer", "user", "other", "") for k in range(nparents)] + [("doc", "d", "owner", "user", "other", "")]
    with aclgpu.Engine(FOLDERS, device=0) as e:
        e.touch(*rels)
        p, er, fl, hops, absent = prove(aclgpu, e, FOLDERS, rels, ("doc", "d", "hidden", "user", "u", ""))
        assert (p, er, fl) == (PERM_HAS, 0, aclgpu.EXPLAIN_PROOF)
        assert hops[0] == owner and sorted(hops[1:]) == parents and len(hops) == 1 + nparents
        assert sorted(absent) == [("folder", f"f{k}", "view", "user", "u", "") for k in range(nparents)]
        _, _, _, _, raw, _, _ = e.explain_proof_ids(item_ids(e, ("doc", "d", "hidden", "user", "u", "")))
        assert [int(h["flags"]) for h in raw] == [0] + [aclgpu.HOP_SEGMENT] * nparents  # every tupleset hop starts at the doc again
        # `other` owns the doc too, but sees every parent
        want = (PERM_HAS, 0, aclgpu.EXPLAIN_PROOF) if nparents == 0 else (PERM_NO, 0, 0)
        assert prove(aclgpu, e, FOLDERS, rels, ("doc", "d", "hidden", "user", "other", ""))[:3] == want


def test_intersection_arrow_over_three_parents(aclgpu):
    rels = []
    for k in range(3):
        rels += [("doc", "d", "parent", "folder", f"f{k}", ""), ("folder", f"f{k}", "viewer", "user", "u", "")]
    rels += [("folder", "f0", "viewer", "user", "v", ""), ("folder", "f1", "viewer", "user", "v", "")]
    with aclgpu.Engine(FOLDERS, device=0) as e:
        e.touch(*rels)
        p, er, fl, hops, absent = prove(aclgpu, e, FOLDERS, rels, ("doc", "d", "shared", "user", "u", ""))
        assert (p, er, fl) == (PERM_HAS, 0, aclgpu.EXPLAIN_PROOF) and absent == []
        assert hops == rels[:6]  # parent, its viewer, parent, its viewer, ...: three chains
        assert prove(aclgpu, e, FOLDERS, rels, ("doc", "d", "shared", "user", "v", "")) == (PERM_NO, 0, 0, [], [])
        assert e.explain_proof("doc", "nothing-above", "shared", "user", "u") == (PERM_NO, 0, 0, [])  # .all() over no parent grants nothing


PARDON = """
definition user {}
definition group {
  relation member: user
}
definition doc {
  relation viewer: user | user:* | group#member
  relation banned: user | group#member
  relation pardoned: user
  permission view = viewer - (banned - pardoned)
}
"""


def test_a_pardon_is_a_hop_and_leaves_no_absence(aclgpu):
    rels = [("doc", "d", "viewer", "user", "u", ""), ("doc", "d", "banned", "user", "u", ""), ("doc", "d", "pardoned", "user", "u", ""),
            ("doc", "d", "viewer", "user", "v", ""), ("doc", "d", "banned", "user", "v", ""), ("doc", "d", "viewer", "user", "w", "")]
    with aclgpu.Engine(PARDON, device=0) as e:
        e.touch(*rels)
        p, er, fl, hops, absent = prove(aclgpu, e, PARDON, rels, ("doc", "d", "view", "user", "u", ""))
        assert (p, er, fl) == (PERM_HAS, 0, aclgpu.EXPLAIN_PROOF) and hops == [rels[0], rels[2]] and absent == []
        assert prove(aclgpu, e, PARDON, rels, ("doc", "d", "view", "user", "v", "")) == (PERM_NO, 0, 0, [], [])
        # w was never banned: the absence of the ban is enough, nobody asks about a pardon
        p, er, fl, hops, absent = prove(aclgpu, e, PARDON, rels, ("doc", "d", "view", "user", "w", ""))
        assert fl == aclgpu.EXPLAIN_PROOF and hops == [rels[5]] and absent == [("doc", "d", "banned", "user", "w", "")]


def test_a_wildcard_viewer_under_an_exclusion_carries_the_flag(aclgpu):
    rels = [("doc", "open", "viewer", "user", "*", ""), ("doc", "open", "banned", "user", "v", "")]
    with aclgpu.Engine(PARDON, device=0) as e:
        e.touch(*rels)
        e.touch(("doc", "elsewhere", "viewer", "user", "u", ""))  # (u is a name the engine knows)
        rels.append(("doc", "elsewhere", "viewer", "user", "u", ""))
        p, er, fl, hops, absent = prove(aclgpu, e, PARDON, rels, ("doc", "open", "view", "user", "u", ""))
        assert (p, er, fl) == (PERM_HAS, 0, aclgpu.EXPLAIN_PROOF) and hops == [rels[0]] and absent == [("doc", "open", "banned", "user", "u", "")]
        _, _, _, _, raw, _, _ = e.explain_proof_ids(item_ids(e, ("doc", "open", "view", "user", "u", "")))
        assert int(raw[0]["flags"]) == aclgpu.HOP_WILDCARD and int(raw[0]["sid"]) == e.find("user", "*")
        assert prove(aclgpu, e, PARDON, rels, ("doc", "open", "view", "user", "v", "")) == (PERM_NO, 0, 0, [], [])


def test_a_subject_that_carries_a_relation(aclgpu):
    rels = [("doc", "d", "viewer", "group", "g", "member"), ("group", "g", "member", "user", "u", ""), ("doc", "e", "viewer", "group", "g", "member"),
            ("doc", "e", "banned", "group", "g", "member")]
    with aclgpu.Engine(PARDON, device=0) as e:
        e.touch(*rels)
        p, er, fl, hops, absent = prove(aclgpu, e, PARDON, rels, ("doc", "d", "view", "group", "g", "member"))
        assert (p, er, fl) == (PERM_HAS, 0, aclgpu.EXPLAIN_PROOF) and hops == [rels[0]] and absent == [("doc", "d", "banned", "group", "g", "member")]
        assert prove(aclgpu, e, PARDON, rels, ("doc", "e", "view", "group", "g", "member")) == (PERM_NO, 0, 0, [], [])
        p, er, fl, hops, absent = prove(aclgpu, e, PARDON, rels, ("doc", "d", "view", "user", "u", ""))
        assert fl == aclgpu.EXPLAIN_PROOF and hops == rels[:2] and absent == [("doc", "d", "banned", "user", "u", "")]


# ---------------------------------------------------------------- 3. nested non-monotone usersets
NEST = """
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


def nest_chain(n):
    return ([("doc", "d", "viewer", "group", "g0", "active")] + [("group", f"g{i}", "member", "group", f"g{i + 1}", "active") for i in range(n)] +
            [("group", f"g{n}", "member", "user", "u", "")])


def test_a_chain_of_groups_gives_one_absence_per_level(aclgpu):
    item = ("doc", "d", "view", "user", "u", "")
    rels = nest_chain(4)  # g0 .. g4
    with aclgpu.Engine(NEST, device=0) as e:
        e.touch(*rels)
        p, er, fl, hops, absent = prove(aclgpu, e, NEST, rels, item)
        assert (p, er, fl) == (PERM_HAS, 0, aclgpu.EXPLAIN_PROOF) and hops == rels
        assert sorted(absent) == [("group", f"g{i}", "banned", "user", "u", "") for i in range(5)]
        # a ban halfway: NO, and nothing comes back
        ban = ("group", "g2", "banned", "user", "u", "")
        e.touch(ban)
        rels.append(ban)
        assert prove(aclgpu, e, NEST, rels, item) == (PERM_NO, 0, 0, [], [])
        # a second path around the ban: the proof takes it
        around = [("group", "g1", "member", "group", "h", "active"), ("group", "h", "member", "user", "u", "")]
        e.touch(*around)
        rels += around
        p, er, fl, hops, absent = prove(aclgpu, e, NEST, rels, item)
        assert fl == aclgpu.EXPLAIN_PROOF and hops == nest_chain(4)[:2] + around
        assert sorted(absent) == [("group", g, "banned", "user", "u", "") for g in ("g0", "g1", "h")]


def test_a_confirmed_candidate_that_leads_back_into_the_path_is_dropped_for_the_next(aclgpu):
    """g1's row holds g0 (a cycle: g0's own Check answers HAS, through g1) and g2 (the way out): the proof does not go round"""
    item = ("doc", "d", "view", "user", "u", "")
    rels = [("doc", "d", "viewer", "group", "g0", "active"), ("group", "g0", "member", "group", "g1", "active"), ("group", "g1", "member", "group", "g0", "active"),
            ("group", "g1", "member", "group", "g2", "active"), ("group", "g2", "member", "user", "u", "")]
    with aclgpu.Engine(NEST, device=0) as e:
        e.touch(*rels)
        assert e.find("group", "g0") < e.find("group", "g2")  # (the cycle's candidate comes first in g1's row)
        p, er, fl, hops, absent = prove(aclgpu, e, NEST, rels, item)
        assert (p, er, fl) == (PERM_HAS, 0, aclgpu.EXPLAIN_PROOF) and hops == [rels[0], rels[1], rels[3], rels[4]]
        assert sorted(absent) == [("group", g, "banned", "user", "u", "") for g in ("g0", "g1", "g2")]
        # and from inside the cycle
        p, er, fl, hops, absent = prove(aclgpu, e, NEST, rels, ("group", "g1", "active", "user", "u", ""))
        assert fl == aclgpu.EXPLAIN_PROOF and hops == rels[3:]


# ---------------------------------------------------------------- 4. the depth limit
def test_the_depth_limit_on_nested_exclusions(aclgpu):
    item = ("doc", "d", "view", "user", "u", "")

    def oracles(n):
        py, c = PyOracle(NEST), orc.Oracle(NEST)
        for r in nest_chain(n):
            py.touch(*r)
        c.touch(*nest_chain(n))
        return py.check(*item), c.check(*item)

    n = max(k for k in range(8, 40) if oracles(k) == (HAS, (PERM_HAS, 0)))
    deeper = oracles(n + 1)
    assert deeper[0] == ERR and deeper[1][1] == aclgpu.ERR_DEPTH
    rels = nest_chain(n)
    with aclgpu.Engine(NEST, device=0) as e:
        e.touch(*rels)
        p, er, fl, hops, absent = prove(aclgpu, e, NEST, rels, item)  # (held to the checker's own count of dispatches)
        assert (p, er, fl) == (PERM_HAS, 0, aclgpu.EXPLAIN_PROOF) and hops == rels and len(absent) == n + 1
    rels = nest_chain(n + 1)
    with aclgpu.Engine(NEST, device=0) as e:
        e.touch(*rels)
        p, er, fl, hops, absent = prove(aclgpu, e, NEST, rels, item)
        assert er == aclgpu.ERR_DEPTH and (p, er) == e.check(*item) and (fl, hops, absent) == (0, [], [])


def test_the_depth_limit_on_a_monotone_stretch_beneath_an_exclusion(aclgpu):
    """`view = viewer - banned` over a chain of plain nested groups: the stretch from doc#viewer to the user is one walk (k_explain_local), whose chain has
    to fit the dispatches that are left beneath the exclusion -- the longest chain both oracles grant is proved, one group more is the depth error"""
    schema = """
definition user {}
definition group {
  relation member: user | group#member
}
definition doc {
  relation viewer: group#member
  relation banned: user
  permission view = viewer - banned
}
"""
    item = ("doc", "d", "view", "user", "u", "")

    def chain(n):
        return ([("doc", "d", "viewer", "group", "g0", "member")] + [("group", f"g{i}", "member", "group", f"g{i + 1}", "member") for i in range(n)] +
                [("group", f"g{n}", "member", "user", "u", "")])

    def oracles(n):
        py, c = PyOracle(schema), orc.Oracle(schema)
        for r in chain(n):
            py.touch(*r)
        c.touch(*chain(n))
        return py.check(*item), c.check(*item)

    n = max(k for k in range(30, 60) if oracles(k) == (HAS, (PERM_HAS, 0)))
    assert oracles(n + 1)[0] == ERR
    for k in (3, n):
        with aclgpu.Engine(schema, device=0) as e:
            e.touch(*chain(k))
            p, er, fl, hops, absent = prove(aclgpu, e, schema, chain(k), item)
            assert (p, er, fl) == (PERM_HAS, 0, aclgpu.EXPLAIN_PROOF) and hops == chain(k) and absent == [("doc", "d", "banned", "user", "u", "")]
    with aclgpu.Engine(schema, device=0) as e:
        e.touch(*chain(n + 1))
        p, er, fl, hops, absent = prove(aclgpu, e, schema, chain(n + 1), item)
        assert er == aclgpu.ERR_DEPTH and (fl, hops, absent) == (0, [], [])


# ---------------------------------------------------------------- 5. randomised parity
MIXED = """
definition user {}
definition group {
  relation member: user | group#active
  relation banned: user
  permission active = member - banned
}
definition folder {
  relation viewer: user | user:* | group#active
  relation banned: user
  relation pardoned: user
  permission view = viewer - (banned - pardoned)
}
definition doc {
  relation owner: user
  relation parent: folder
  relation blocked: user
  permission every = parent.all(view)
  permission both = owner & parent->view
  permission open = (owner + parent->view) - blocked
  permission hidden = owner - parent->view
  permission lonely = owner - parent.all(view)
}
"""
MIXED_PERMS = [("group", "active"), ("folder", "view"), ("doc", "every"), ("doc", "both"), ("doc", "open"), ("doc", "hidden"), ("doc", "lonely")]
N_USER, N_GROUP, N_FOLDER, N_DOC = 8, 6, 5, 6


def mixed_graph(seed):
    """8 users, 6 groups nested through `active` (cycles allowed), 5 folders, 6 docs with 0 .. 5 parents"""
    rng = random.Random(seed)
    users, groups = [f"u{k}" for k in range(N_USER)], [f"g{k}" for k in range(N_GROUP)]
    folders, docs = [f"f{k}" for k in range(N_FOLDER)], [f"d{k}" for k in range(N_DOC)]
    rels = set()
    for g in groups:
        for u in users:
            if rng.random() < 0.25:
                rels.add(("group", g, "member", "user", u, ""))
            if rng.random() < 0.10:
                rels.add(("group", g, "banned", "user", u, ""))
        for h in groups:
            if h != g and rng.random() < 0.2:
                rels.add(("group", g, "member", "group", h, "active"))
    for f in folders:
        if rng.random() < 0.3:
            rels.add(("folder", f, "viewer", "user", "*", ""))
        for u in users:
            if rng.random() < 0.2:
                rels.add(("folder", f, "viewer", "user", u, ""))
            if rng.random() < 0.25:
                rels.add(("folder", f, "banned", "user", u, ""))
                if rng.random() < 0.4:
                    rels.add(("folder", f, "pardoned", "user", u, ""))
        for g in groups:
            if rng.random() < 0.25:
                rels.add(("folder", f, "viewer", "group", g, "active"))
    for d in docs:
        for u in users:
            if rng.random() < 0.45:
                rels.add(("doc", d, "owner", "user", u, ""))
            if rng.random() < 0.15:
                rels.add(("doc", d, "blocked", "user", u, ""))
        for f in rng.sample(folders, rng.choice([0, 1, 1, 2, 2, 3, 5])):
            rels.add(("doc", d, "parent", "folder", f, ""))
    # every name exists for the engine (an object nobody names has no id to ask about)
    names = {"user": users, "group": groups, "folder": folders, "doc": docs}
    items = [(t, o, p, "user", u, "") for t, p in MIXED_PERMS for o in names[t] for u in users]
    return sorted(rels), names, items


def mixed_engine(aclgpu, rels, names, named, **cfg):
    e = aclgpu.Engine(MIXED, device=0, **cfg)
    e.touch(*rels)
    for t, objs in names.items():  # objects no relationship names still get an id
        for o in objs:
            if e.find(t, o) is None:
                e.intern(t, o)
    return e, np.concatenate([item_ids(e, it) for it in named])


def test_random_graphs_prove_every_permission_and_the_default_configuration_agrees(aclgpu):
    """Over the family every permission of the schema is proved at least once.  And the same batches through an engine with the DEFAULT max_sub_batch:
    the test below opens its engines with 16, because on the seeds whose groups nest in a cycle under an exclusion the Check of a whole batch visits more
    combine states than one pass holds (acl_check_bulk_ids itself answers RESOURCE_EXHAUSTED).  Where Check answers, the proofs are the same records;
    where it refuses, the proof call refuses with the same code -- it never returns less."""
    proved, refused = set(), 0
    for seed in range(8):
        rels, names, named = mixed_graph(seed)
        e, items = mixed_engine(aclgpu, rels, names, named, max_sub_batch=16)
        with e:
            small = e.explain_proof_ids(items)
        proved |= {(it[0], it[2]) for it, fl in zip(named, small[2]) if int(fl) == aclgpu.EXPLAIN_PROOF}
        e, items = mixed_engine(aclgpu, rels, names, named)
        with e:
            try:
                e.check_bulk_ids(items)
            except aclgpu.AclError as x:
                assert x.code == aclgpu.ERR_RESOURCE_EXHAUSTED
                refused += 1
                with pytest.raises(aclgpu.AclError) as y:
                    e.explain_proof_ids(items)
                assert y.value.code == aclgpu.ERR_RESOURCE_EXHAUSTED
                continue
            big = e.explain_proof_ids(items)
        assert all(np.array_equal(u, v) for u, v in zip(big[:4], small[:4])) and np.array_equal(big[5], small[5])  # answers, flags, offsets
        assert sorted(map(bytes, big[6])) == sorted(map(bytes, small[6]))
    print(f"default max_sub_batch: Check refused {refused} of 8 batches")
    assert proved == set(MIXED_PERMS), sorted(set(MIXED_PERMS) - proved)


@pytest.mark.parametrize("seed", range(8))
def test_random_graphs_every_granted_item_is_proved(aclgpu, seed):
    rels, names, named = mixed_graph(seed)
    chk = P.ProofChecker(MIXED, rels)
    # (groups nested in a cycle under an exclusion: a Check that ends at the depth limit visits a state once per path to it, and a pass holds 2^20 of them)
    e, items = mixed_engine(aclgpu, rels, names, named, max_sub_batch=16)
    with e:
        perm, err, flags, off, raw, aoff, araw = e.explain_proof_ids(items)
        cperm, cerr = e.check_bulk_ids(items)
        assert np.array_equal(perm, cperm) and np.array_equal(err, cerr)
        nm = Names(e, MIXED)
        granted = 0
        for i, it in enumerate(named):
            want = chk.py.check(*it)
            cp, ce = chk.c.check(*it)
            assert (int(perm[i]), int(err[i])) == (cp, ce), (it, int(perm[i]), int(err[i]), cp, ce)
            assert want == {PERM_HAS: HAS, PERM_NO: NO}.get(int(perm[i]) if not err[i] else -1, ERR), (it, want)
            hops, absent = nm.hops(raw[off[i]:off[i + 1]]), nm.absent(araw[aoff[i]:aoff[i + 1]])
            assert int(flags[i]) != aclgpu.EXPLAIN_UNSUPPORTED
            if int(perm[i]) == PERM_HAS and not err[i]:
                assert int(flags[i]) == aclgpu.EXPLAIN_PROOF, it  # (every permission of this schema is non-monotone)
                chk.check(it, hops, absent)
                segments_ok(aclgpu, raw[off[i]:off[i + 1]])
                granted += 1
            else:
                assert int(flags[i]) == 0 and hops == [] and absent == [], it
        # without these an empty answer could pass: a fifth of every batch is granted ...
        print(f"seed {seed}: {granted} of {len(named)} granted, {len(raw)} hops, {len(araw)} absences")
        assert granted * 5 >= len(named), (granted, len(named))

# ---------------------------------------------------------------- 6. overflow and size
def wide_group(aclgpu, e, n):
    e.add_edges("group", "member", "group", "active", np.zeros(n, dtype=np.uint32), np.arange(1, n + 1, dtype=np.uint32))
    e.add_edges("group", "member", "user", "", [n], [0])
    e.add_edges("doc", "viewer", "group", "active", [0], [0])
    items = e.make_items("doc", "view", [0], "user", "", [0])
    perm, err = e.check_bulk_ids(items)
    assert (int(perm[0]), int(err[0])) == (PERM_HAS, 0)
    return items


def test_a_row_of_20000_nested_groups(aclgpu):
    n = 20000
    with aclgpu.Engine(NEST, device=0) as e:
        items = wide_group(aclgpu, e, n)
        perm, err, flags, off, raw, aoff, araw = e.explain_proof_ids(items)
        assert (int(perm[0]), int(err[0]), int(flags[0])) == (PERM_HAS, 0, aclgpu.EXPLAIN_PROOF)
        nm = Names(e, NEST, named=False)
        want = [("doc", "0", "viewer", "group", "0", "active"), ("group", "0", "member", "group", str(n), "active"), ("group", str(n), "member", "user", "0", "")]
        assert nm.hops(raw) == want
        assert sorted(nm.absent(araw)) == sorted([("group", "0", "banned", "user", "0", ""), ("group", str(n), "banned", "user", "0", "")])
        P.check_proof(NEST, want, ("doc", "0", "view", "user", "0", ""), nm.hops(raw), nm.absent(araw))


def test_a_row_of_20000_nested_groups_redoes_an_overflowed_region(aclgpu):
    """the 20 000 members of the row are enumerated on the device into a region that starts at 2^14 ids: the pass is redone with a larger one, as Explain's
    walk redoes a chunk (test_overflow_retry), and the call's own Checks overflow nothing"""
    n = 20000
    with aclgpu.Engine(NEST, device=0) as e:
        items = wide_group(aclgpu, e, n)
        s0 = e.stats()["overflow_retries"]
        perm, err, flags, off, raw, aoff, araw = e.explain_proof_ids(items)
        s1 = e.stats()["overflow_retries"]
        assert int(flags[0]) == aclgpu.EXPLAIN_PROOF and len(raw) == 3
        print(f"overflow_retries: {s0} -> {s1}")
        assert s1 > s0


def test_a_thousand_parents_give_a_thousand_absences(aclgpu):
    n = 1000
    with aclgpu.Engine(FOLDERS, device=0) as e:
        e.add_edges("doc", "owner", "user", "", [0], [0])
        e.add_edges("doc", "parent", "folder", "", np.zeros(n, dtype=np.uint32), np.arange(n, dtype=np.uint32))
        e.add_edges("folder", "viewer", "user", "", np.arange(n, dtype=np.uint32), np.ones(n, dtype=np.uint32))
        items = e.make_items("doc", "hidden", [0, 0], "user", "", [0, 1])
        perm, err, flags, off, raw, aoff, araw = e.explain_proof_ids(items)
        assert perm.tolist() == [PERM_HAS, PERM_NO] and not err.any() and flags.tolist() == [aclgpu.EXPLAIN_PROOF, 0]
        assert off.tolist() == [0, n + 1, n + 1] and aoff.tolist() == [0, n, n]
        nm = Names(e, FOLDERS, named=False)
        hops, absent = nm.hops(raw), nm.absent(araw)
        assert hops[0] == ("doc", "0", "owner", "user", "0", "") and sorted(hops[1:]) == sorted(("doc", "0", "parent", "folder", str(k), "") for k in range(n))
        assert sorted(absent) == sorted(("folder", str(k), "view", "user", "0", "") for k in range(n))
        rels = hops + [("folder", str(k), "viewer", "user", "1", "") for k in range(n)]
        P.check_proof(FOLDERS, rels, ("doc", "0", "hidden", "user", "0", ""), hops, absent)


def test_a_proof_beyond_the_record_limit_is_refused_not_truncated(aclgpu):
    n = aclgpu.PROOF_MAX_RECORDS + 1
    with aclgpu.Engine(FOLDERS, device=0) as e:
        e.add_edges("doc", "owner", "user", "", [0, 1], [0, 0])
        e.add_edges("doc", "parent", "folder", "", np.zeros(n, dtype=np.uint32), np.arange(n, dtype=np.uint32))
        e.add_edges("doc", "parent", "folder", "", [1], [0])
        perm, err = e.check_bulk_ids(e.make_items("doc", "hidden", [0], "user", "", [0]))
        assert (int(perm[0]), int(err[0])) == (PERM_HAS, 0)
        with pytest.raises(aclgpu.AclError) as x:
            e.explain_proof_ids(e.make_items("doc", "hidden", [1, 0], "user", "", [0, 0]))
        assert x.value.code == aclgpu.ERR_RESOURCE_EXHAUSTED and "item 1 " in str(x.value)
        # the small item on its own is proved
        perm, err, flags, off, raw, aoff, araw = e.explain_proof_ids(e.make_items("doc", "hidden", [1], "user", "", [0]))
        assert flags.tolist() == [aclgpu.EXPLAIN_PROOF] and len(raw) == 2 and len(araw) == 1


# ---------------------------------------------------------------- 7. writes and time
def test_deleting_a_hop_moves_the_proof_or_denies_the_item(aclgpu):
    item = ("doc", "d", "view", "user", "u", "")
    rels = [("doc", "d", "viewer", "group", "a", "active"), ("group", "a", "member", "user", "u", ""),
            ("doc", "d", "viewer", "group", "b", "active"), ("group", "b", "member", "user", "u", "")]
    with aclgpu.Engine(NEST, device=0) as e:
        e.touch(*rels)
        live = list(rels)
        _, _, fl, first, absent = prove(aclgpu, e, NEST, live, item)
        assert fl == aclgpu.EXPLAIN_PROOF and len(first) == 2 and len(absent) == 1
        e.write([(aclgpu.OP_DELETE, first[1])])
        live.remove(first[1])
        _, _, fl, second, absent = prove(aclgpu, e, NEST, live, item)  # (held to the checker against what is stored NOW)
        assert fl == aclgpu.EXPLAIN_PROOF and len(second) == 2 and not set(second) & set(first)
        e.write([(aclgpu.OP_DELETE, second[1])])
        live.remove(second[1])
        assert prove(aclgpu, e, NEST, live, item) == (PERM_NO, 0, 0, [], [])


def test_adding_the_relationship_an_absence_names_denies_the_item(aclgpu):
    item = ("doc", "d", "view", "user", "u", "")
    rels = nest_chain(1)
    with aclgpu.Engine(NEST, device=0) as e:
        e.touch(*rels)
        _, _, fl, hops, absent = prove(aclgpu, e, NEST, rels, item)
        assert fl == aclgpu.EXPLAIN_PROOF and len(absent) == 2
        for a in absent:
            e.touch(a)  # the absent goal is a relation here: the absence names a relationship
            assert prove(aclgpu, e, NEST, rels + [a], item) == (PERM_NO, 0, 0, [], [])
            e.write([(aclgpu.OP_DELETE, a)])
        assert prove(aclgpu, e, NEST, rels, item)[2] == aclgpu.EXPLAIN_PROOF


def test_an_expired_hop_is_in_no_proof(aclgpu):
    schema = """
definition user {}
definition group {
  relation member: user
}
definition pod {
  relation viewer: user with expiration | group#member
  relation banned: user with expiration
  permission view = viewer - banned
}
"""
    item = ("pod", "p", "view", "user", "u", "")
    direct = ("pod", "p", "viewer", "user", "u", "")
    long = [("pod", "p", "viewer", "group", "g", "member"), ("group", "g", "member", "user", "u", "")]
    ban = ("pod", "p", "banned", "user", "u", "")
    absent_ban = [ban]
    with aclgpu.Engine(schema, device=0) as e:
        e.set_now(100)
        e.touch(*long)
        e.write([(aclgpu.OP_TOUCH, direct, 1000)])
        _, _, fl, hops, absent = prove(aclgpu, e, schema, long + [direct], item)
        assert fl == aclgpu.EXPLAIN_PROOF and hops == [direct] and absent == absent_ban
        e.set_now(1000)  # the direct grant has run out
        _, _, fl, hops, absent = prove(aclgpu, e, schema, long, item)
        assert fl == aclgpu.EXPLAIN_PROOF and hops == long and absent == absent_ban
        e.write([(aclgpu.OP_TOUCH, ban, 2000)])  # a ban that runs out: denied while it lasts, absent again afterwards
        assert prove(aclgpu, e, schema, long + [ban], item) == (PERM_NO, 0, 0, [], [])
        e.set_now(2000)
        _, _, fl, hops, absent = prove(aclgpu, e, schema, long, item)
        assert fl == aclgpu.EXPLAIN_PROOF and hops == long and absent == absent_ban


# ---------------------------------------------------------------- 8. shapes
def test_batch_shapes(aclgpu, aclgpu_lib):
    rels = [("doc", "d", "viewer", "user", "a", ""), ("doc", "d", "viewer", "user", "b", ""), ("doc", "d", "banned", "user", "b", ""), ("doc", "d", "editor", "user", "a", "")]
    named = [("doc", "d", "view", "user", "a", ""), ("doc", "d", "edit", "user", "a", ""), ("doc", "d", "view", "user", "b", ""), ("doc", "d", "edit", "user", "b", "")]
    want = [(aclgpu.EXPLAIN_PROOF, [rels[0]], [("doc", "d", "banned", "user", "a", "")]), (aclgpu.EXPLAIN_WITNESS, [rels[3]], []), (0, [], []), (0, [], [])]
    with aclgpu.Engine(BAN, device=0, max_sub_batch=256) as e:
        e.touch(*rels)
        out = e.explain_proof_ids(np.zeros(0, dtype=aclgpu.ITEM_DTYPE))  # n = 0
        assert all(a.size == 0 for a in (out[0], out[1], out[2], out[4], out[6])) and out[3].tolist() == [0] and out[5].tolist() == [0]
        for it, (fl, hops, absent) in zip(named, want):  # n = 1, both entry points
            assert prove(aclgpu, e, BAN, rels, it)[2:] == (fl, hops, absent)
        # names nobody wrote: answered as Check answers them, nothing proved
        for it in (("doc", "d", "view", "user", "nobody-wrote-this", ""), ("doc", "no-such-doc", "view", "user", "a", "")):
            p, er, fl, lines = e.explain_proof(*it)
            assert (p, er) == e.check(*it) == (PERM_NO, 0) and fl == 0 and lines == []
        p, er, fl, lines = e.explain_proof("doc", "d", "nope", "user", "a")
        assert (p, er) == e.check("doc", "d", "nope", "user", "a") and er == aclgpu.ERR_FAILED_PRECONDITION and fl == 0 and lines == []
        with pytest.raises(aclgpu.AclError) as x:
            e.explain_proof("doc", "not an id", "view", "user", "a")
        assert x.value.code == aclgpu.ERR_INVALID_ARGUMENT
        # 1 025 items over a sub-batch of 256: monotone, non-monotone, denied and ids without relationships mixed
        ghost_user, ghost_doc = e.intern("user", "ghost"), e.intern("doc", "ghost")
        one = [item_ids(e, it) for it in named] + [e.make_items("doc", "view", [e.find("doc", "d")], "user", "", [ghost_user]),
                                                   e.make_items("doc", "view", [ghost_doc], "user", "", [e.find("user", "a")])]
        want += [(0, [], []), (0, [], [])]
        pick = np.arange(1025) % len(one)
        items = np.concatenate(one)[pick]
        perm, err, flags, off, raw, aoff, araw = e.explain_proof_ids(items)
        cperm, cerr = e.check_bulk_ids(items)
        assert np.array_equal(perm, cperm) and np.array_equal(err, cerr) and off[-1] == raw.size and aoff[-1] == araw.size
        nm = Names(e, BAN)
        for i, k in enumerate(pick):
            assert (int(flags[i]), nm.hops(raw[off[i]:off[i + 1]]), nm.absent(araw[aoff[i]:aoff[i + 1]])) == want[k], (i, k)
        # acl_call_opts_t: already cancelled / already past its deadline are refused; a live flag and a generous deadline change nothing
        import ctypes
        flag = ctypes.c_int32(1)
        with pytest.raises(aclgpu.AclError) as x:
            e.explain_proof_ids(items, cancel=flag)
        assert x.value.code == aclgpu.ERR_CANCELLED
        with pytest.raises(aclgpu.AclError) as x:
            e.explain_proof_ids(items, timeout_s=1e-9)
        assert x.value.code == aclgpu.ERR_DEADLINE_EXCEEDED
        flag.value = 0
        again = e.explain_proof_ids(items, cancel=flag, timeout_s=60.0)
        assert all(np.array_equal(u, v) for u, v in zip(again, (perm, err, flags, off, raw, aoff, araw)))
        # one shard of a sharded graph does not prove
        e._check(aclgpu_lib.acl_shard_configure(e._h, 0, 2))
        with pytest.raises(aclgpu.AclError) as x:
            e.explain_proof_ids(items[:4])
        assert x.value.code == aclgpu.ERR_FAILED_PRECONDITION

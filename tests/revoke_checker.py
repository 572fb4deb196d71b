"""The checker of Explain for revocation (acl_explain_revoke*): the one place that holds an answer to the oracles.

It works from the test's own relationship set and both oracles (tests/denial_checker.py's Oracles: oracle/orc.py's C oracle and PyOracle), never from the
engine.  For one granted item and the cuts an engine reported for it:

1. every cut is a stored relationship, live at the oracles' `now`, listed once;
2. sound: with that one relationship deleted, the Python oracle and the C oracle both answer something other than HAS;
3. complete: for EVERY relationship of the store that is not listed, the C oracle still answers HAS with it deleted -- the brute force;
4. the Python oracle repeats the brute force for the unlisted hops of a witness (the caller takes it from explain_ids on the same engine and validates it
   with explain_checker.check_witness first): those are the only relationships a wrong answer could plausibly have dropped.

Checker.brute() runs the brute force of step 3 for many items at once (one delete, every item asked, one touch back per relationship) and keeps the result;
check() reads it from there when it has the item, and runs it for the one item when it has not."""
import random

from oracle import orc
from tests import denial_checker as D

ORC_HAS = D.ORC_HAS


def hop_tuples(hops):
    return [tuple(h[:6]) for h in hops]


class Checker:
    def __init__(self, schema, rels, now=0):
        self.orcs = D.Oracles(schema, rels, now)
        self._cuts = {}  # item -> frozenset of the relationships whose delete the C oracle answers with something other than HAS

    # ---- one relationship out, and back as it was
    def _out(self, r):
        self.orcs.c.write([(orc.OP_DELETE, r)])
        self.orcs.py.delete(*r)

    def _back(self, r):
        self.orcs.probe_off(r)

    def live(self, r):
        exp = self.orcs.rels.get(r)
        return exp is not None and (exp == 0 or exp > self.orcs.now)

    def granted(self, item):
        (p, e), y = self.orcs.check(item)
        return p == ORC_HAS and e == 0 and y == "HAS"

    def brute(self, items, only=None):
        """{item: frozenset(cuts)} by the C oracle alone, for the items both oracles grant (every other item is left out); only: the relationships to try
        (default: every relationship of the store)"""
        items = [it for it in dict.fromkeys(items) if self.granted(it)]
        todo = [it for it in items if it not in self._cuts]
        if todo or only is not None:
            found = {it: set() for it in (items if only is not None else todo)}
            for r in (list(self.orcs.rels) if only is None else only):
                self.orcs.c.write([(orc.OP_DELETE, r)])
                try:
                    for it in found:
                        if self.orcs.c.check(*it)[0] != ORC_HAS:
                            found[it].add(r)
                finally:
                    self.orcs.c.write([(orc.OP_TOUCH, r, self.orcs.rels[r])])
            if only is not None:
                return {it: frozenset(s) for it, s in found.items()}
            for it, s in found.items():
                self._cuts[it] = frozenset(s)
        return {it: self._cuts[it] for it in items}

    def check(self, item, cuts, witness=None, sample=None, seed=0):
        """item: (rtype, rid, perm, stype, sid, srel); cuts: the relationships the engine listed for it, 6-tuples (`*` spells a wildcard's id); witness: hops
        of a validated witness of the item.  sample: hold completeness to that many unlisted relationships, drawn at random, plus the witness's (a store of
        tens of thousands of relationships; None: all of them)."""
        assert self.granted(item), f"{item} is not granted by both oracles"
        cuts = hop_tuples(cuts)
        assert len(set(cuts)) == len(cuts), f"a relationship is listed twice: {cuts}"
        for r in cuts:
            assert r in self.orcs.rels, f"cut {r} is not a stored relationship"
            assert self.live(r), f"cut {r} is not live"
            self._out(r)
            try:
                (p, e), y = self.orcs.check(item)
                assert p != ORC_HAS and y != "HAS", f"deleting {r} does not revoke {item}: {(p, e, y)}"
            finally:
                self._back(r)
        listed = set(cuts)
        hops = [r for r in dict.fromkeys(hop_tuples(witness or ())) if r not in listed]
        if sample is None:
            want = self.brute([item])[item]
        else:
            rest = [r for r in self.orcs.rels if r not in listed]
            only = list(dict.fromkeys(hops + (rest if len(rest) <= sample else random.Random(seed).sample(rest, sample))))
            want = self.brute([item], only=only)[item] | listed
        missing = sorted(want - listed)
        assert not missing, f"deleting {missing[0]} revokes {item}, and it is not listed ({len(missing)} such)"
        for r in hops:
            assert r in self.orcs.rels, f"hop {r} of the witness is not a stored relationship"
            self._out(r)
            try:
                assert self.orcs.py.check(*item) == "HAS", f"deleting the witness's hop {r} revokes {item} (PyOracle), and it is not listed"
            finally:
                self._back(r)
        assert self.granted(item)


# ---- the random graphs of tests/test_explain_revoke_gpu.py: nested groups and arrows (folders above docs, folders above folders), a wildcard class
NESTED = """
definition user {}
definition group {
  relation member: user | group#member
}
definition folder {
  relation parent: folder
  relation viewer: user | group#member
  permission view = viewer + parent->view
}
definition doc {
  relation folder: folder
  relation viewer: user | user:* | group#member
  relation editor: user | group#member
  permission edit = editor
  permission view = viewer + edit + folder->view
}
"""
SEEDS = [0, 1, 2, 5, 6, 8, 10, 12]  # picked on the CPU: random_case()'s conditions hold for each (14 of the first 20 seeds do)


def random_graph(seed):
    """(relationships, candidate items): groups nest downwards only and folders hang under later folders only, so no Check errs"""
    rnd = random.Random(f"revoke/{seed}")
    nu, ng, nf, nd = 24, 48, 28, 48
    users, groups = [f"u{i}" for i in range(nu)], [f"g{i}" for i in range(ng)]
    folders, docs = [f"f{i}" for i in range(nf)], [f"d{i}" for i in range(nd)]
    rels = []
    for i, g in enumerate(groups):
        rels += [("group", g, "member", "user", u, "") for u in rnd.sample(users, rnd.randint(0, 4))]
        later = groups[i + 1:]
        rels += [("group", g, "member", "group", h, "member") for h in rnd.sample(later, min(len(later), rnd.randint(0, 2)))]
    for i, f in enumerate(folders):
        later = folders[i + 1:]
        rels += [("folder", f, "parent", "folder", p, "") for p in rnd.sample(later, min(len(later), rnd.randint(0, 2)))]
        rels += [("folder", f, "viewer", "group", g, "member") for g in rnd.sample(groups, rnd.randint(0, 1))]
        if rnd.random() < 0.4:
            rels.append(("folder", f, "viewer", "user", rnd.choice(users), ""))
    for d in docs:
        rels += [("doc", d, "folder", "folder", f, "") for f in rnd.sample(folders, rnd.randint(0, 2))]
        for rel in ("viewer", "editor"):
            rels += [("doc", d, rel, "group", g, "member") for g in rnd.sample(groups, rnd.randint(0, 2))]
            if rnd.random() < 0.3:
                rels.append(("doc", d, rel, "user", rnd.choice(users), ""))
        if rnd.random() < 0.1:
            rels.append(("doc", d, "viewer", "user", "*", ""))
    rels = list(dict.fromkeys(rels))
    items = [("doc", d, "view", "user", u, "") for d in docs for u in users]
    items += [("folder", f, "view", "user", u, "") for f in folders[:8] for u in users]
    items += [("doc", d, "view", "group", g, "member") for d in docs[:12] for g in groups]
    items += [("doc", d, "edit", "user", u, "") for d in docs[:8] for u in users]
    return rels, items


def random_case(seed):
    """(Checker, granted items, {item: cuts}) of random_graph(seed): the brute force over all relationships x all granted items, by the oracles alone, and
    the conditions the seeds are picked for, asserted here so that no test on these graphs can go vacuous -- at least a quarter of the granted items have
    a cut and at least a quarter have none"""
    rels, items = random_graph(seed)
    ck = Checker(NESTED, rels)
    want = ck.brute(items)
    granted = list(want)
    with_cut = sum(bool(c) for c in want.values())
    assert len(granted) >= 200 and 4 * with_cut >= len(granted) and 4 * (len(granted) - with_cut) >= len(granted), (seed, len(granted), with_cut)
    return ck, granted, want

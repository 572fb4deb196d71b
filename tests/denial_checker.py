"""The checker of Explain for denials (acl_explain_denial*): a restatement on the CPU, and the one place that holds an answer to the oracles.

Written against oracle/pyoracle.py's parsed schema and a plain dict of relationships {(rtype, rid, rel, stype, sid, srel): expires_at (0 = never)}:

1. closure(): the states (type, id, relation or permission) a Check of R#P looks at, each with the least dispatch level it is reached at -- breadth first
   over references on the same object, live userset subjects and arrow targets, up to the 50 dispatches of a Check.  Monotone schemas only.
2. grants_of(): from the closure, the relationships `o#r@subject` that a subject of one class could be written into.
3. check_grants(): an engine's answer is held to BOTH oracles (oracle/orc.py's C oracle and PyOracle), never to the closure above: every reported grant,
   written alone, makes both answer HAS, at exactly the reported level; every other relationship with that subject that the schema allows does not."""
import random

from oracle import orc
from oracle.pyoracle import HAS, MAX_DEPTH, PyOracle, Relation, parse_schema

ORC_HAS, ORC_NO = 2, 1


def as_dict(rels):
    """relationships as {6-tuple: expires_at}: accepts that dict, or an iterable of 6-tuples / (6-tuple..., expires) 7-tuples"""
    if isinstance(rels, dict):
        return dict(rels)
    return {tuple(r[:6]): (r[6] if len(r) > 6 else 0) for r in rels}


def closure(defs, rels, root, now=0, refs=True):
    """{(type, id, member): least level} of the Check of root = (type, id, member).  refs=False leaves out the states that are reached, at their least level,
    by a reference alone: what a walk returns whose programs inline every computed userset (their arrows and usersets are still followed)."""
    rows = {}
    for (rt, rid, rel, st, sid, sr), exp in as_dict(rels).items():
        if exp == 0 or exp > now:
            rows.setdefault((rt, rid, rel), []).append((st, sid, sr))
    level = {root: 1}
    by_ref_only = {root: False}
    frontier = [root]
    for lv in range(1, MAX_DEPTH):
        nxt = []

        def reach(state, by_ref):
            if state not in level:
                level[state] = lv + 1
                by_ref_only[state] = by_ref
                nxt.append(state)
            elif level[state] == lv + 1 and not by_ref:
                by_ref_only[state] = False

        for (t, o, m) in frontier:
            mem = defs[t].members[m]
            if isinstance(mem, Relation):
                for (st, sid, sr) in rows.get((t, o, m), ()):
                    if sr and sr != "*" and sid != "*":
                        reach((st, sid, sr), False)
                continue
            todo = [mem.expr]
            while todo:
                e = todo.pop()
                if e[0] == "union":
                    todo += [e[1], e[2]]
                elif e[0] == "ref":
                    reach((t, o, e[1]), True)
                elif e[0] == "arrow":
                    for (st, sid, _sr) in rows.get((t, o, e[1]), ()):
                        if e[2] in defs[st].members:
                            reach((st, sid, e[2]), False)
                else:
                    assert e[0] == "nil", f"closure(): {e[0]} is not monotone"
        frontier = nxt
    return level if refs else {s: lv for s, lv in level.items() if not by_ref_only[s]}


def accepts(mem, stype, srel):
    """a relation that takes a named subject of class stype[#srel] (a `T:*` form does not count)"""
    return isinstance(mem, Relation) and any(a[0] == stype and a[1] != "*" and (a[1] or "") == srel for a in mem.allowed)


def grants_of(defs, clos, stype, srel=""):
    """{(rtype, rid, relation): level} for a subject of class stype[#srel], from a closure WITH its reference states (refs=True)"""
    return {(t, o, m): lv for (t, o, m), lv in clos.items() if accepts(defs[t].members[m], stype, srel)}


class Oracles:
    """both oracles over one schema, loaded with the same relationships"""

    def __init__(self, schema, rels=(), now=0):
        self.schema = schema
        self.c = orc.Oracle(schema)
        self.py = PyOracle(schema)
        self.defs = self.py.defs
        self.now = now
        self.c.set_now(now)
        self.py.now = now
        self.rels = {}
        self.touch_all(as_dict(rels))

    def touch_all(self, rels):
        items = list(as_dict(rels).items())
        for b in range(0, len(items), 1000):
            self.c.write([(orc.OP_TOUCH, r, exp) for r, exp in items[b:b + 1000]])
        for r, exp in items:
            self.py.touch(*r, expires=exp)
            self.rels[r] = exp

    def probe_on(self, r):
        self.c.write([(orc.OP_TOUCH, r, 0)])
        self.py.touch(*r, expires=0)

    def probe_off(self, r):
        """the relationship as it was before the probe: gone, or back with the expiry it had"""
        if r in self.rels:
            self.c.write([(orc.OP_TOUCH, r, self.rels[r])])
            self.py.touch(*r, expires=self.rels[r])
        else:
            self.c.write([(orc.OP_DELETE, r)])
            self.py.delete(*r)

    def check(self, item):
        """(C oracle's (permissionship, error), PyOracle's 'HAS' | 'NO' | 'ERR')"""
        return self.c.check(*item), self.py.check(*item)

    def denied(self, item):
        (p, e), y = self.check(item)
        return p == ORC_NO and e == 0 and y == "NO"

    def grants_with_budget(self, item, d):
        """PyOracle's recursion with a depth budget of d dispatches (its _check with a depth argument, the memo reset per call)"""
        rt, rid, perm, st, sid, srel = item
        self.py._memo = {}
        return self.py._check(rt, rid, perm, (st, sid, srel), d) == HAS

    def least_budget(self, item):
        """the least depth budget with which PyOracle's recursion grants the item (None: none up to 50)"""
        for d in range(1, MAX_DEPTH + 1):
            if self.grants_with_budget(item, d):
                return d
        return None

    def objects(self):
        objs = set()
        for (rt, rid, _rel, st, sid, _sr) in self.rels:
            objs.add((rt, rid))
            if sid != "*":
                objs.add((st, sid))
        return objs


def check_grants(orcs, item, grants, others=True, seed=0):
    """item: (rtype, rid, perm, stype, sid, srel); grants: [(rtype, rid, relation, level)] as the engine reported them for it.  orcs: Oracles holding the
    relationships the engine was asked on.  others=False: soundness and levels of `grants` only (a sample of a large answer; its completeness is the
    caller's to establish)."""
    rt, rid, perm, st, sid, srel = item
    assert orcs.denied(item), f"{item} is not denied without error by both oracles"
    keys = [(g[0], g[1], g[2]) for g in grants]
    assert len(set(keys)) == len(keys), "a relationship is listed twice"
    for (gt, gid, grel, level) in grants:
        r = (gt, gid, grel, st, sid, srel)
        assert accepts(orcs.defs[gt].members[grel], st, srel), f"{r}: the schema does not allow it"
        orcs.probe_on(r)
        try:
            (p, e), y = orcs.check(item)
            assert (p, e, y) == (ORC_HAS, 0, "HAS"), f"writing {r} does not grant {item}: {(p, e, y)}"
            # (a larger budget never takes a grant away on a monotone schema, so "granted with `level`, not with `level - 1`" says that `level` is the least)
            assert 1 <= level <= MAX_DEPTH and orcs.grants_with_budget(item, level) and not orcs.grants_with_budget(item, level - 1), \
                f"{r}: level {level} reported, PyOracle grants from depth budget {orcs.least_budget(item)}"
        finally:
            orcs.probe_off(r)
    if not others:
        return
    listed = set(keys)
    rest = []
    for (ot, oid) in sorted(orcs.objects() | {(rt, rid)}):
        for name, mem in orcs.defs[ot].members.items():
            if accepts(mem, st, srel) and (ot, oid, name) not in listed:
                rest.append((ot, oid, name, st, sid, srel))
    sample = set(rest if len(rest) <= 200 else random.Random(seed).sample(rest, 200))
    for r in rest:
        orcs.probe_on(r)
        try:
            p, e = orcs.c.check(*item)
            assert p != ORC_HAS, f"writing {r} grants {item}, and it is not listed"
            if r in sample:
                assert orcs.py.check(*item) != "HAS", f"writing {r} grants {item} (PyOracle), and it is not listed"
        finally:
            orcs.probe_off(r)
    assert orcs.denied(item)


def slot_table(e, schema):
    """{(type, member): slot} of an engine over `schema`: the type's first slot + member index, types and members in declaration order"""
    defs = parse_schema(schema)
    out, base = {}, 0
    for ti, (t, d) in enumerate(defs.items()):
        assert e.type_id(t) == ti
        for mi, m in enumerate(d.members):
            assert e.relation_id(t, m) == mi
            out[(t, m)] = base + mi
        base += len(d.members)
    return out


def encode_states(e, slots, clos):
    """a closure as the records acl_selfcheck_denial_grants takes: [(object id, slot | level << 16)] (every object known to the engine)"""
    return [(e.find(t, o), slots[(t, m)] | (lv << 16)) for (t, o, m), lv in clos.items()]


def name_grants(e, schema, recs):
    """acl_grant_t records -> [(rtype, rid, relation, level)] by name, in the records' order (asserted to be the contract's: level, rtype, relation, rid)"""
    defs = parse_schema(schema)
    tname = {e.type_id(t): t for t in defs}
    out = []
    keys = [(int(g["level"]), int(g["rtype"]), int(g["relation"]), int(g["rid"])) for g in recs]
    assert keys == sorted(keys), "grants are not sorted by (level, rtype, relation, rid)"
    for g in recs:
        t = tname[int(g["rtype"])]
        out.append((t, e.object_name(t, int(g["rid"])), list(defs[t].members)[int(g["relation"])], int(g["level"])))
    return out


# ---- the random graphs of tests/test_explain_denial_cpu.py and tests/test_explain_denial_gpu.py: two monotone families, 12 to 40 objects
GROUPS = """
definition user {}
definition group {
  relation member: user | group#member
  relation admin: user
}
definition doc {
  relation viewer: user | group#member
  relation editor: user | group#member
  relation owner: user
  permission edit = editor + owner
  permission view = viewer + edit
}
"""
HIERARCHY = """
definition user {}
definition org {
  relation admin: user
  relation member: user
  permission view = admin + member
}
definition folder {
  relation org: org
  relation viewer: user
  permission view = viewer + org->view
}
definition doc {
  relation folder: folder
  relation viewer: user
  relation creator: user
  permission view = viewer + creator + folder->view
}
"""
# a permission of more operands than one program inlines (plan.cpp: 256 ops a slot): the references past that point are states of their own (OP_PUSH_SAME)
PUSHED_RELATIONS = 260
PUSHED = ("definition user {}\ndefinition group {\n  relation member: user | group#member\n}\ndefinition doc {\n" +
          "".join(f"  relation r{i}: user\n" for i in range(PUSHED_RELATIONS)) + "  relation viewer: user | group#member\n  permission tail = viewer\n  permission big = " +
          " + ".join(f"r{i}" for i in range(PUSHED_RELATIONS)) + " + tail\n}\n")
FAMILIES = {"groups": GROUPS, "hierarchy": HIERARCHY}
SEEDS = list(range(8))


def random_graph(family, seed):
    """(schema, relationships dict, candidate items): 12 to 40 objects; the groups nest downwards only (group i holds groups j > i), so no Check errs"""
    rnd = random.Random(f"{family}/{seed}")
    rels = {}
    if family == "groups":
        nu, ng, nd = rnd.randint(4, 12), rnd.randint(4, 16), rnd.randint(4, 12)
        users, groups, docs = [f"u{i}" for i in range(nu)], [f"g{i}" for i in range(ng)], [f"d{i}" for i in range(nd)]
        for i, g in enumerate(groups):
            for u in rnd.sample(users, rnd.randint(0, 2)):
                rels[("group", g, "member", "user", u, "")] = 0
            for j in range(i + 1, ng):
                if rnd.random() < 0.3:
                    rels[("group", g, "member", "group", groups[j], "member")] = 0
        for d in docs:
            for rel in ("viewer", "editor"):
                for g in rnd.sample(groups, rnd.randint(0, 2)):
                    rels[("doc", d, rel, "group", g, "member")] = 0
            if rnd.random() < 0.5:
                rels[("doc", d, "owner", "user", rnd.choice(users), "")] = 0
        items = [("doc", d, "view", "user", u, "") for d in docs for u in users + ["nobody"]]
        items += [("doc", d, "view", "group", g, "member") for d in docs for g in groups[:4]]
        items += [("doc", d, "edit", "user", u, "") for d in docs[:3] for u in users[:3]]
    else:
        nu, no, nf, nd = rnd.randint(4, 10), rnd.randint(2, 5), rnd.randint(3, 10), rnd.randint(3, 15)
        users, orgs = [f"u{i}" for i in range(nu)], [f"o{i}" for i in range(no)]
        folders, docs = [f"f{i}" for i in range(nf)], [f"d{i}" for i in range(nd)]
        for o in orgs:
            rels[("org", o, "admin", "user", rnd.choice(users), "")] = 0
            if rnd.random() < 0.5:
                rels[("org", o, "member", "user", rnd.choice(users), "")] = 0
        for f in folders:
            for o in rnd.sample(orgs, rnd.randint(1, 2)):
                rels[("folder", f, "org", "org", o, "")] = 0
            if rnd.random() < 0.4:
                rels[("folder", f, "viewer", "user", rnd.choice(users), "")] = 0
        for d in docs:
            for f in rnd.sample(folders, rnd.randint(1, 2)):
                rels[("doc", d, "folder", "folder", f, "")] = 0
            if rnd.random() < 0.4:
                rels[("doc", d, "creator", "user", rnd.choice(users), "")] = 0
        items = [("doc", d, "view", "user", u, "") for d in docs for u in users + ["nobody"]]
        items += [("folder", f, "view", "user", u, "") for f in folders[:3] for u in users[:3]]
    rnd.shuffle(items)
    return FAMILIES[family], rels, items


def denied_items(orcs, items, want=24):
    """the first `want` of `items` that both oracles deny without error, and the condition the random graphs are chosen for: at least 20 of them, at least
    10 with a grant, at least 5 with a grant at level 3 or more -- established on the oracle side, before any engine is asked"""
    out = []
    for it in items:
        if orcs.denied(it):
            out.append(it)
            if len(out) == want:
                break
    assert len(out) >= 20, f"only {len(out)} denied items"
    with_grant = deep = 0
    for it in out:
        g = grants_of(orcs.defs, closure(orcs.defs, orcs.rels, it[:3], orcs.now), it[3], it[5])
        with_grant += bool(g)
        deep += any(lv >= 3 for lv in g.values())
    assert with_grant >= 10 and deep >= 5, (with_grant, deep)
    return out

"""A seeded generator of random schemas with a small universe over each: what tests/test_random_schema_cpu.py and tests/test_random_schema_gpu.py hold
the plan compiler (plan.cpp, plan_reverse.cpp, plan_subjects.cpp) and the walks to the two oracles on.  Plain random.Random -- the same arguments give
the same case on every machine -- and no engine anywhere: a case is text, tuples of strings and nothing else.

Shape of a schema: `definition user {}` plus 2-4 definitions of 2-4 relations and 2-4 permissions each.  The first relation of a definition is its
TUPLESET: it allows plain objects of one or two types, and arrows (`ts->m`, `ts.any(m)`, `ts.all(m)`) go over tuplesets only -- that keeps arrows away
from wildcard and userset subjects, whose semantics both oracles mark as unverified.  `ts.all(m)` is drawn only where every subject type of `ts` has
`m` (the engine and both oracles refuse the other case at load); `ts->m` and `ts.any(m)` need `m` on one of them.  The other relations allow 1-3 of
`user`, `user:*`, `T`, `T#relation`, `T#permission`.  A permission is a random tree of depth <= 3 over `+` (weighted), `&` and `-` with random
parentheses; its leaves are `nil` (rare), relations and permissions of its definition, and arrows.

Modes:
  monotone   only `+`, `->`, `.any()` and `nil`: the plain kernel instantiations and the Explain family
  general    everything; a permission refers only to permissions declared above it
  recursive  as general, and a permission may refer to any permission of its definition, itself included
  wide       a general schema over 40 objects per type and 100 users (rows cross 32-bit words and 64-lane windows); held to the C oracle only

CYCLIC_SHARE of the relationships whose subject is an object are drawn freely; the others point from an object to one of a lower rank, so they alone
close no cycle.  Cycles are what ends a Check in the depth error.  Two rules shape them:
  - no case holds a BRANCHING cycle through a combining permission (branching_cycle below): the engine's contract is to refuse such a Check with
    RESOURCE_EXHAUSTED where the oracles memoise it, so there is nothing to compare.  A schema whose references alone make one, and a relationship
    that would close one, are drawn again.  The rule was found by this generator: without it the engine refused 15 of the 42 corpus seeds, exactly
    the 15 that branching_cycle names, and agreed with the oracles on all others.
  - a branching cycle through monotone members makes the single-launch walk overflow and hand over to the level loop (and costs the Python oracle
    seconds): BRANCHY_SHARE of the seeds may hold one, the others hold simple cycles only."""
import random
from collections import namedtuple

MODES = ("monotone", "general", "recursive", "wide")
SMALL_MODES = MODES[:3]
CORPUS = {"monotone": tuple(range(12)), "general": tuple(range(12)), "recursive": tuple(range(12)), "wide": tuple(range(6))}
CYCLIC_SHARE = 0.5
BRANCHY_SHARE = 0.5  # of the seeds may hold a branching cycle through monotone members
NOBODY = "nobody"  # the user no relationship names

TYPE_NAMES = ("org", "team", "folder", "doc")
REL_NAMES = ("parent", "viewer", "editor", "owner")         # the first one is every definition's tupleset
PERM_NAMES = ("view", "edit", "admin", "audit")

Case = namedtuple("Case", "seed mode schema rels rounds users subjects items lookup_subjects lookup_targets types members allowed")
Case.__doc__ = """schema: text; rels: the initial relationships, 6-tuples (rtype, rid, rel, stype, sid, srel); rounds: three (deletes, touches) pairs of 6-tuples, each
to be applied on top of the one before; subjects: (stype, sid, srel); items: Check 6-tuples; lookup_subjects: the four subjects of LookupResources;
lookup_targets: (rtype, member, stype, sid, srel); types: {type: [object names]} (user included); members: {type: [member names in slot order]};
allowed: {(type, relation): [(stype, srel or "" or "*")]}"""


def corpus(modes=SMALL_MODES):
    return [(m, s) for m in modes for s in CORPUS[m]]


def _gen_schema(rng, mode):
    monotone = mode == "monotone"
    recursive = mode == "recursive"
    types = rng.sample(TYPE_NAMES, rng.randint(2, 4))
    rels = {t: list(REL_NAMES[:rng.randint(2, 4)]) for t in types}
    perms = {t: list(PERM_NAMES[:rng.randint(2, 4)]) for t in types}
    members = {t: rels[t] + perms[t] for t in types}
    allowed = {}
    for t in types:
        allowed[(t, "parent")] = [(x, "") for x in rng.sample(types, rng.randint(1, 2))]
        for r in rels[t][1:]:
            forms = []
            for _ in range(rng.randint(1, 3)):
                k = rng.random()
                if k < 0.35:
                    f = ("user", "")
                elif k < 0.50:
                    f = ("user", "*")
                elif k < 0.60:
                    f = (rng.choice(types), "")
                elif k < 0.80:  # (half of these nest the relation in itself, as groups of groups do: `member: user | group#member`)
                    x = rng.choice(types)
                    f = (t, r) if rng.random() < 0.5 else (x, rng.choice(rels[x]))
                else:
                    x = rng.choice(types)
                    f = (x, rng.choice(perms[x]))
                if f not in forms:
                    forms.append(f)
            allowed[(t, r)] = forms

    def leaf(t, k):
        x = rng.random()
        if x < 0.04:
            return "nil"
        if x < 0.40:
            return rng.choice(rels[t])
        if x < 0.62:
            pool = perms[t] if recursive else perms[t][:k]
            return rng.choice(pool) if pool else rng.choice(rels[t])
        stypes = [s for s, _ in allowed[(t, "parent")]]
        on_any = sorted({m for s in stypes for m in members[s]})
        on_all = sorted(m for m in on_any if all(m in members[s] for s in stypes))
        form = rng.random()
        if not monotone and on_all and form < 0.30:
            return f"parent.all({rng.choice(on_all)})"
        m = rng.choice(on_any)
        return f"parent.any({m})" if form < 0.60 else f"parent->{m}"

    def tree(t, k, depth):
        if depth == 0 or rng.random() < 0.30:
            return leaf(t, k), False
        x = rng.random()
        op = "+" if monotone or x < 0.50 else "&" if x < 0.75 else "-"
        parts = []
        for _ in range(2):
            text, compound = tree(t, k, depth - 1)
            # (a compound operand keeps its own grouping, which the parsers' precedence would otherwise regroup, half of the time)
            parts.append(f"({text})" if compound and rng.random() < 0.5 else text)
        return f"{parts[0]} {op} {parts[1]}", True

    lines = ["definition user {}"]
    for t in types:
        lines.append(f"definition {t} {{")
        for r in rels[t]:
            forms = " | ".join(s + (":*" if m == "*" else f"#{m}" if m else "") for s, m in allowed[(t, r)])
            lines.append(f"  relation {r}: {forms}")
        for k, p in enumerate(perms[t]):
            lines.append(f"  permission {p} = {tree(t, k, 3)[0]}")
        lines.append("}")
    return "\n".join(lines) + "\n", types, members, allowed


def _rand_rel(rng, types, objects, allowed, users):
    """one valid relationship, or None when the draw does not fit the acyclic ranking"""
    (t, r), forms = rng.choice(sorted(allowed.items()))
    s, m = rng.choice(forms)
    oi = rng.randrange(len(objects[t]))
    if s == "user":
        return (t, objects[t][oi], r, "user", "*" if m == "*" else rng.choice(users), "")
    si = rng.randrange(len(objects[s]))
    if rng.random() >= CYCLIC_SHARE:  # rank = (object index, type index): the subject's must be the lower one
        ti, tsi = types.index(t), types.index(s)
        if (si, tsi) > (oi, ti):
            oi, si = si, oi
        if (si, tsi) >= (oi, ti):
            return None
    return (t, objects[t][oi], r, s, objects[s][si], m)


def gen(seed, mode):
    assert mode in MODES, mode
    rng = random.Random(f"random-schema/{mode}/{seed}")
    wide = mode == "wide"
    from oracle.pyoracle import parse_schema
    while True:  # (a schema whose references alone make a branching cycle through a combining permission is drawn again: see branching_cycle)
        schema, types, members, allowed = _gen_schema(rng, "general" if wide else mode)
        defs = parse_schema(schema)
        if branching_cycle(defs, (), [(t, "x") for t in types]) is None:
            break
    branchy = rng.random() < BRANCHY_SHARE
    n_obj, n_user = (40, 100) if wide else (3, 4)
    objects = {t: [f"{t[0]}{i}" for i in range(n_obj)] for t in types}
    users = [f"u{i}" for i in range(n_user)]

    def fits(rs):
        return branching_cycle(defs, rs, monotone_too=not branchy) is None

    def draw(n, have):
        out = []
        for _ in range(200 * n):  # (a tiny schema may not have n relationships left to draw)
            if len(out) == n:
                break
            r = _rand_rel(rng, types, objects, allowed, users)
            if r is None or r in have or r in out:
                continue
            if r[3] != "user" and not fits(live_of(have) + out + [r]):
                continue  # (only a relationship onto an object adds a way)
            out.append(r)
        return out

    gone = []

    def live_of(have):
        return [r for r in have if r not in gone]

    rels = draw(rng.randint(150, 400) if wide else rng.randint(8, 40), [])
    live, rounds = list(rels), []
    for _ in range(3):
        deletes = rng.sample(live, min(len(live) - 1, rng.randint(2, 4)))
        live = [r for r in live if r not in deletes]
        gone = deletes
        touches = draw(rng.randint(2, 4), live + deletes)  # (one write may not name a relationship twice)
        live += touches
        rounds.append((deletes, touches))

    usersets = []
    while len(usersets) < 3:
        t = rng.choice(types)
        s = (t, rng.choice(objects[t]), rng.choice(members[t]))
        if s not in usersets:
            usersets.append(s)
    subjects = [("user", u, "") for u in users + [NOBODY]] + usersets
    every = [(t, o, m) for t in types for o in objects[t] for m in members[t]]
    if wide:  # (every triple would be 10^5 Checks a seed: a seeded sample -- a third of it asked by the userset subjects, a third by anybody, and a
        #        third by the subject of a relationship about a member of that relationship's resource, so that grants are no rarity)
        items = []
        for k in range(3000):
            r = rng.choice(rels)
            if k % 3 == 2 and r[4] != "*":
                items.append((r[0], r[1], rng.choice(members[r[0]])) + r[3:])
            else:
                items.append(rng.choice(every) + (rng.choice(subjects) if k % 3 else rng.choice(usersets)))
    else:
        items = [q + s for q in every for s in subjects]
    lookup_subjects = [("user", u, "") for u in rng.sample(users, 2)] + rng.sample(usersets, 2)
    lookup_targets = [(t, m) + s for t in types for m in members[t] for s in lookup_subjects]
    all_objects = dict(objects, user=users + [NOBODY])
    return Case(seed, mode, schema, rels, rounds, users, subjects, items, lookup_subjects, lookup_targets, all_objects, members, allowed)


def _leaves(e):
    if e[0] in ("union", "inter", "excl"):
        return _leaves(e[1]) + _leaves(e[2])
    return [e]


def _nonmonotone(e):
    return e[0] in ("inter", "excl", "arrow_all") or (e[0] == "union" and (_nonmonotone(e[1]) or _nonmonotone(e[2])))


def combine_members(defs):
    """{(type, permission)} whose own evaluation combines verdicts: `-`, `&` or `.all()` in its expression, or in that of a permission of its
    definition it refers to (a reference is evaluated on the same object, as part of the referring permission)"""
    from oracle.pyoracle import Permission
    out = {(t, m) for t, d in defs.items() for m, mem in d.members.items() if isinstance(mem, Permission) and _nonmonotone(mem.expr)}
    changed = True
    while changed:
        changed = False
        for t, d in defs.items():
            for m, mem in d.members.items():
                if (t, m) not in out and isinstance(mem, Permission) and any(x[0] == "ref" and (t, x[1]) in out for x in _leaves(mem.expr)):
                    out.add((t, m))
                    changed = True
    return out


def _dispatch_graph(defs, rels, objects=()):
    """{state: [states a Check of it dispatches to, one entry per way]} over `rels`; a state is (type, object, member)"""
    from oracle.pyoracle import Relation
    rows = {}
    for (rt, rid, rel, st, sid, srel) in rels:
        if sid != "*":
            rows.setdefault((rt, rid, rel), []).append((st, sid, srel))
    objects = set(objects) | {(r[0], r[1]) for r in rels} | {(r[3], r[4]) for r in rels if r[3] in defs and r[4] != "*"}
    edges = {}
    for (t, o) in sorted(objects):
        for m, mem in defs[t].members.items():
            out = []
            if isinstance(mem, Relation):
                out = [s for s in rows.get((t, o, m), ()) if s[2]]
            else:
                for x in _leaves(mem.expr):
                    if x[0] == "ref":
                        out.append((t, o, x[1]))
                    elif x[0] in ("arrow", "arrow_all"):
                        out += [(st, sid, x[2]) for (st, sid, _sr) in rows.get((t, o, x[1]), ()) if x[2] in defs[st].members]
            edges[(t, o, m)] = out
    return edges


def branching_cycle(defs, rels, objects=(), monotone_too=False):
    """A state (type, object, member) of the Check's dispatch graph over `rels` that lies on a cycle through a combining permission (combine_members)
    and has two ways on within that cycle's component -- or None.  Both oracles memoise such a graph; a walk that gives every visit of a combining
    state verdict cells of its own doubles them per level there, and the engine's contract is to refuse such a Check loudly
    (tests/test_combine_gpu.py test_branching_cycles_under_exclusion_and_intersection).  A cycle through a combining permission that does not
    branch, and any cycle through monotone members only, is within the contract and is generated.
    monotone_too: look for a branching cycle through any members at all.  defs: oracle.pyoracle.parse_schema's; objects: (type, object) pairs to look at besides those the relationships name"""
    edges = _dispatch_graph(defs, rels, objects)
    combining = combine_members(defs)
    # Tarjan's strongly connected components, iteratively (a wide case has more states than the interpreter allows frames)
    index, low, on, stack, comp_of, n = {}, {}, set(), [], {}, 0
    for root in edges:
        if root in index:
            continue
        work = [(root, iter(edges.get(root, ())))]
        index[root] = low[root] = n
        n += 1
        stack.append(root)
        on.add(root)
        while work:
            v, it = work[-1]
            for w in it:
                if w not in index:
                    index[w] = low[w] = n
                    n += 1
                    stack.append(w)
                    on.add(w)
                    work.append((w, iter(edges.get(w, ()))))
                    break
                if w in on:
                    low[v] = min(low[v], index[w])
            else:
                work.pop()
                if work:
                    low[work[-1][0]] = min(low[work[-1][0]], low[v])
                if low[v] == index[v]:
                    while True:
                        w = stack.pop()
                        on.discard(w)
                        comp_of[w] = v
                        if w == v:
                            break
    comps = {}
    for v, c in comp_of.items():
        comps.setdefault(c, []).append(v)
    for c, vs in comps.items():
        inside = {v: [w for w in edges.get(v, ()) if comp_of.get(w) == c] for v in vs}
        if not any(inside.values()) or not (monotone_too or any((v[0], v[2]) in combining for v in vs)):
            continue  # (no cycle here, or a monotone one)
        for v in sorted(vs):
            if len(inside[v]) > 1:
                return v
    return None


def live_after(case, n_rounds):
    """the relationships after the first n_rounds write rounds, in a fixed order"""
    live = list(case.rels)
    for deletes, touches in case.rounds[:n_rounds]:
        live = [r for r in live if r not in deletes] + list(touches)
    return live


# ---- what the CPU and the GPU file share: the corpus' cases, generated once, and the oracles over a relationship set
SMALL = corpus()
IDS = [f"{m}-{s}" for m, s in SMALL]
_cases = {}


def case_of(mode, seed):
    if (mode, seed) not in _cases:
        _cases[(mode, seed)] = gen(seed, mode)
    return _cases[(mode, seed)]


def load_oracles(schema, rels, python=True):
    """(C oracle, Python oracle or None) over `rels`"""
    from oracle import orc
    from oracle.pyoracle import PyOracle
    co, po = orc.Oracle(schema), PyOracle(schema) if python else None
    for k in range(0, len(rels), 500):
        co.write([(orc.OP_TOUCH, r) for r in rels[k:k + 500]])
    for r in rels if python else ():
        po.touch(*r)
    return co, po

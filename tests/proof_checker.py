"""The one checker every Explain proof is held to (tests/test_explain_proof_gpu.py; its own behaviour is checked on the CPU by
tests/test_explain_proof_cpu.py).

A proof of a granted item is a list of hops -- stored relationships (rtype, rid, rel, stype, sid, srel), a wildcard hop names the subject id "*" -- and a list
of absences, Check items (rtype, rid, rel, stype, sid, srel) with the item's own subject.  With S the stored relationships, H the hops as a set and N the
absent goals (rtype, rid, rel):
  - H is a subset of S;
  - every goal of N answers NO on S by both oracles;
  - the item derives by the rules below, positive steps reading relationships from H only, within 50 dispatches counted as oracle/pyoracle.py counts them.

  expression        derive                                                          refute (inside a subtracted operand)
  state == subject  holds                                                           -
  relation r of o   H holds o#r@subject, or o#r@T:* for a plain subject of type T,  (o, r) is in N
                    or a userset hop o#r@x#s and state (x, s) derives
  ref r             state (o, r) derives, one dispatch down                         (o, r) is in N
  a + b             either                                                          both
  a & b             both                                                            either
  a - b             derive a and refute b                                           refute a, or derive b
  t->p              some o#t@x in H with (x, p) deriving                            for every o#t@x in S, (x, p) is in N
  t.all(p)          S holds at least one o#t@x; every such hop is in H and          S holds none, or some (x, p) is in N
                    every (x, p) derives
  nil               never                                                           always
and an absence reached through a tupleset has that tupleset relationship among the hops: a refutation under `t->p` needs every o#t@x in H, one under
`t.all(p)` the hop o#t@x of the parent it names."""
from oracle import orc
from oracle.pyoracle import NO, MAX_DEPTH, PyOracle, Relation, parse_schema


class ProofChecker:
    """The oracles over one relationship set, built once; check() holds one proof to the contract."""

    def __init__(self, schema, relationships, now=0):
        """relationships: 6-tuples, (6-tuple..., expires_at) 7-tuples or {6-tuple: expires_at}; now: the clock of both oracles.  S is what is live then, and
        every relationship is written with its expiry."""
        self.defs = parse_schema(schema)
        at = dict(relationships) if isinstance(relationships, dict) else {tuple(r[:6]): (r[6] if len(r) > 6 else 0) for r in relationships}
        self.S = {r for r, exp in at.items() if exp == 0 or exp > now}
        self.py, self.c = PyOracle(schema), orc.Oracle(schema)
        self.py.now = now
        self.c.set_now(now)
        for r, exp in at.items():
            self.py.touch(*r, expires=exp)
        todo = sorted(at.items())
        for k in range(0, len(todo), 500):  # (a write holds at most 1 000 updates)
            self.c.write([(orc.OP_TOUCH, r, exp) for r, exp in todo[k:k + 500]])
        self.rows = {}
        for r in self.S:
            self.rows.setdefault(r[:3], set()).add(r[3:6])

    def check(self, item, hops, absent):
        rt, rid, perm, st, sid, srel = item
        subject = (st, sid, srel)
        H = {tuple(h[:6]) for h in hops}
        for h in H:
            assert h in self.S, f"hop {h} is not a stored relationship"
        N = set()
        for a in absent:
            a = tuple(a[:6])
            assert a[3:6] == subject, f"absence {a} does not ask about the item's subject {subject}"
            p, c = self.py.check(*a), self.c.check(*a)
            assert p == NO, f"Python oracle: the absent goal {a} answers {p}"
            assert c == (1, 0), f"C oracle: the absent goal {a} answers {c}"
            N.add(a[:3])
        hrows = {}
        for h in H:
            hrows.setdefault(h[:3], set()).add(h[3:6])
        defs, srows, memo = self.defs, self.rows, {}

        def members(rows, t, o, ts, p):
            return sorted(s for s in rows.get((t, o, ts), ()) if p in defs[s[0]].members)

        def derive_state(t, o, r, d):
            key = (t, o, r, d)
            if key not in memo:
                memo[key] = False  # (a derivation through its own goal at the same depth is none)
                memo[key] = state_body(t, o, r, d)
            return memo[key]

        def state_body(t, o, r, d):
            if d <= 0:
                return False
            if subject == (t, o, r):
                return True
            mem = defs[t].members[r]
            if isinstance(mem, Relation):
                subs = hrows.get((t, o, r), ())
                if subject in subs or (srel == "" and (st, "*", "") in subs):
                    return True
                return any(s[2] and derive_state(s[0], s[1], s[2], d - 1) for s in sorted(subs))
            return derive(mem.expr, t, o, d)

        def derive(e, t, o, d):
            k = e[0]
            if k == "nil":
                return False
            if k == "union":
                return derive(e[1], t, o, d) or derive(e[2], t, o, d)
            if k == "inter":
                return derive(e[1], t, o, d) and derive(e[2], t, o, d)
            if k == "excl":
                return derive(e[1], t, o, d) and refute(e[2], t, o, d)
            if k == "ref":
                return derive_state(t, o, e[1], d - 1)
            if k == "arrow":
                return any(derive_state(x[0], x[1], e[2], d - 1) for x in members(hrows, t, o, e[1], e[2]))
            assert k == "arrow_all", e
            every = members(srows, t, o, e[1], e[2])
            return bool(every) and all(x in hrows.get((t, o, e[1]), ()) and derive_state(x[0], x[1], e[2], d - 1) for x in every)

        def refute(e, t, o, d):
            k = e[0]
            if k == "nil":
                return True
            if k == "union":
                return refute(e[1], t, o, d) and refute(e[2], t, o, d)
            if k == "inter":
                return refute(e[1], t, o, d) or refute(e[2], t, o, d)
            if k == "excl":
                return refute(e[1], t, o, d) or derive(e[2], t, o, d)
            if k == "ref":
                return (t, o, e[1]) in N
            every = members(srows, t, o, e[1], e[2])
            led = hrows.get((t, o, e[1]), ())  # the tupleset hops that lead the reader to the absences
            if k == "arrow":
                return all((x[0], x[1], e[2]) in N and x in led for x in every)
            assert k == "arrow_all", e
            return not every or any((x[0], x[1], e[2]) in N and x in led for x in every)

        assert derive_state(rt, rid, perm, MAX_DEPTH), f"{item} does not derive from hops {sorted(H)} and absences {sorted(N)}"


def check_proof(schema, relationships, item, hops, absent):
    """item: (rt, rid, perm, st, sid, srel); relationships: the stored 6-tuples; hops, absent: the proof.  Raises AssertionError when it is none."""
    ProofChecker(schema, relationships).check(item, hops, absent)

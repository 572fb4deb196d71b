"""The LookupSubjects contract by the Python oracle: one copy for tests/test_lookup_subjects_gpu.py, tests/test_sharded_subjects_gpu.py and the read
campaign of tools/fuzz_gpu.py (run_reads).

ids = {s : Relaxed'(s) == HAS and Check(s) == HAS}, where Relaxed' is the Check under the positive relaxation of the schema (`a - b` -> a, `a & b` -> a + b,
`a.all(b)` -> a->b) on the relationships minus the `T:*` ones; wildcard = Relaxed(fresh) == HAS and Check(fresh) == HAS for a subject nobody names;
excluded = {s : Check(s) != HAS} when wildcard; a reached subject whose Check errs fails the call with ACL_ERR_DEPTH (ACL_FLAG_LENIENT_LOOKUP: it is
left out)."""
from oracle.pyoracle import ERR, HAS, PyOracle


class SubjectsContract:
    """The three oracles of the contract over one relationship set and one subject type, loaded once: answer() is contract() for one resource.
    rels: [(rt, rid, rel, st, sid, srel, expires)]"""

    def __init__(self, schema, rels, st, now=0):
        self.st = st
        self.full, self.relaxed, self.relaxed_w = PyOracle(schema), PyOracle(schema), PyOracle(schema)
        for r in rels:
            self.full.touch(*r[:6], expires=r[6] if len(r) > 6 else 0)
            self.relaxed_w.touch(*r[:6], expires=r[6] if len(r) > 6 else 0)
            if not (r[3] == st and r[4] == "*"):
                self.relaxed.touch(*r[:6], expires=r[6] if len(r) > 6 else 0)
        for o in (self.full, self.relaxed, self.relaxed_w):
            o.now = now
        self.relaxed.relaxed = self.relaxed_w.relaxed = True

    def answer(self, rt, rid, perm, srel, names, lenient=False):
        """(ids, wildcard, excluded) or the string "DEPTH" when the call must fail"""
        full, relaxed, relaxed_w, st = self.full, self.relaxed, self.relaxed_w, self.st
        fail = False
        ids = set()
        for s in names:
            c, rx = full.check(rt, rid, perm, st, s, srel), relaxed.check(rt, rid, perm, st, s, srel)
            if rx == HAS and c == HAS:
                ids.add(s)
            if rx == HAS and c == ERR and not lenient:
                fail = True
        fresh = "nobody-names-this-subject"
        wild = False
        if not srel and relaxed_w.check(rt, rid, perm, st, fresh) == HAS:
            cf = full.check(rt, rid, perm, st, fresh)
            wild = cf == HAS
            if cf == ERR and not lenient:
                fail = True
        excluded = set()
        if wild:
            for s in names:
                c = full.check(rt, rid, perm, st, s, srel)
                if c != HAS:
                    excluded.add(s)
                    if c == ERR and not lenient:
                        fail = True
        return "DEPTH" if fail else (ids, wild, excluded)


def contract(schema, rels, rt, rid, perm, st, srel, names, lenient=False, now=0):
    """the contract by the Python oracle: (ids, wildcard, excluded) or the string "DEPTH" when the call must fail.
    rels: [(rt, rid, rel, st, sid, srel, expires)]"""
    return SubjectsContract(schema, rels, st, now).answer(rt, rid, perm, srel, names, lenient)

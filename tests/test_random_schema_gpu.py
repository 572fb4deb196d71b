"""Random schemas on the GPU (tests/schema_gen.py): what the plan compiler makes of a schema nobody wrote by hand -- inlined usersets and OP_PUSH_SAME,
mark-through relations, rev_useful / rev_sink, slot_deep, two-hop rows, combine programs, the LookupSubjects states -- executed by the walks and held to
BOTH oracles: Check on the single-launch walk and on the level loop, LookupResources by outcome (failures by code), LookupSubjects by the contract of
tests/subjects_contract.py, all of it again after each of three write rounds, and the Explain family through its checkers.  `wide` seeds (40 objects
per type, 100 users: rows cross 32-bit words and 64-lane windows) are held to the C oracle alone.  Four seeds run on 2 and 3 logical shards.
The oracles' own agreement and the generator's coverage are tests/test_random_schema_cpu.py's."""
import random

import numpy as np
import pytest

from oracle import orc
from tests import denial_checker as D
from tests import explain_checker as X
from tests import proof_checker as P
from tests import revoke_checker as R
from tests import schema_gen as G
from tests.outcomes import outcome
from tests.subjects_contract import SubjectsContract
from tests.test_oracle_cross import PY2C
from tests.schema_gen import SMALL, case_of, load_oracles

pytestmark = pytest.mark.gpu

HAS, NO = (orc.PERM_HAS, 0), (orc.PERM_NO, 0)
WIDE = [("wide", s) for s in G.CORPUS["wide"]]
SHARDED = [("monotone", 0), ("monotone", 1), ("general", 0), ("general", 1)]
_expected = {}
# Seeds the engine refuses where the oracles answer (profiles/random_schema.md): kept in the corpus, at most two.
XFAIL = {
    ("recursive", 2): "RESOURCE_EXHAUSTED where both oracles answer: an item's walk makes more than 2^24 combine nodes; tests/test_combine_gpu.py::test_cycles_chained_above_a_combining_permission",
    ("wide", 2): "RESOURCE_EXHAUSTED where the C oracle answers: an item's walk makes more than 2^24 combine nodes; tests/test_combine_gpu.py::test_cycles_chained_above_a_combining_permission",
}


def params(cases):
    return [pytest.param(m, s, id=f"{m}-{s}", marks=[pytest.mark.xfail(strict=True, reason=XFAIL[(m, s)])] if (m, s) in XFAIL else []) for m, s in cases]


@pytest.fixture(scope="module")
def aclgpu(aclgpu_lib):
    import aclgpu as m
    return m


def nonmono_of(schema):
    """{(type, member)} with `-`, `&` or `.all()` anywhere beneath: a least fixpoint over references, arrows and userset subjects"""
    from oracle.pyoracle import Relation, parse_schema
    defs = parse_schema(schema)
    nm = set()

    def expr(t, x):
        if x[0] in ("inter", "excl", "arrow_all"):
            return True
        if x[0] == "union":
            return expr(t, x[1]) or expr(t, x[2])
        if x[0] == "ref":
            return (t, x[1]) in nm
        if x[0] == "arrow":
            return any((a[0], x[2]) in nm for a in defs[t].members[x[1]].allowed)
        return False

    changed = True
    while changed:
        changed = False
        for t, d in defs.items():
            for m, mem in d.members.items():
                if (t, m) not in nm and (any(a[1] and a[1] != "*" and (a[0], a[1]) in nm for a in mem.allowed) if isinstance(mem, Relation) else expr(t, mem.expr)):
                    nm.add((t, m))
                    changed = True
    return nm


def subject_targets(c):
    """(rtype, member, rid, stype, srel): every (type, member), two resources, subject type `user` and one userset form"""
    ut, _, um = c.subjects[-1]
    out = []
    for k, (t, ms) in enumerate(c.members.items()):
        for j, m in enumerate(ms):
            objs = c.types[t]
            for rid in (objs[(k + j) % 3], objs[(k + j + 1) % 3]):
                out += [(t, m, rid, "user", ""), (t, m, rid, ut, um)]
    return out


def expected(mode, seed, rnd):
    """what both oracles say after `rnd` write rounds: Checks (asserted equal between them), lookup outcomes of both, LookupSubjects contracts.  After a
    write round a third of the lookup and subject targets (every third, starting at the round's number).  Computed once, shared, never modified."""
    key = (mode, seed, rnd)
    if key not in _expected:
        c = case_of(mode, seed)
        rels = G.live_after(c, rnd)
        co, po = load_oracles(c.schema, rels)
        checks = [co.check(*q) for q in c.items]
        assert checks == [PY2C[po.check(*q)] for q in c.items]
        lt, st_ = c.lookup_targets, subject_targets(c)
        if rnd:
            lt, st_ = lt[rnd - 1::3], st_[rnd - 1::3]
        lookups = [(t, outcome(co.lookup, *t), outcome(po.lookup_resources, *t)) for t in lt]
        contracts = {}
        subjects = []
        for (rt, m, rid, st, srel) in st_:
            if st not in contracts:
                contracts[st] = SubjectsContract(c.schema, rels, st)
            subjects.append(((rt, m, rid, st, srel), contracts[st].answer(rt, rid, m, srel, c.types[st])))
        _expected[key] = {"rels": rels, "checks": checks, "lookups": lookups, "subjects": subjects}
    return _expected[key]


def open_engine(aclgpu, c, rels, **kw):
    e = aclgpu.Engine(c.schema, **kw)
    for k in range(0, len(rels), 500):
        e.write([(aclgpu.OP_TOUCH, r) for r in rels[k:k + 500]])
    for t, objs in c.types.items():  # every name of the universe has its id, the user no relationship names included
        for o in objs:
            e.intern(t, o)
    return e


def subjects_answer(aclgpu, e, rt, m, rid, st, srel):
    try:
        return e.lookup_subjects(rt, rid, m, st, srel)
    except aclgpu.AclError as x:
        if x.code != aclgpu.ERR_DEPTH:
            raise
        return "DEPTH"


def compare_reads(aclgpu, e, c, want, where, checks_only=False):
    perms, errs = e.check_bulk(c.items)
    got = list(zip((int(p) for p in perms), (int(x) for x in errs)))
    bad = [(q, g, w) for q, g, w in zip(c.items, got, want["checks"]) if g != w]
    assert not bad, f"{where}: {len(bad)} Checks differ (item, engine, oracles): {bad[:4]}"
    if checks_only:
        return
    for t, cw, pw in want["lookups"]:
        g = outcome(e.lookup, *t)
        assert g == cw == pw, f"{where}: LookupResources {t}: engine {g}, C oracle {cw}, Python oracle {pw}"
    for t, w in want["subjects"]:
        g = subjects_answer(aclgpu, e, *t)
        assert g == w, f"{where}: LookupSubjects {t}: engine {g}, contract {w}"


def item_ids(aclgpu, e, named):
    out = np.zeros(len(named), dtype=aclgpu.ITEM_DTYPE)
    for i, (rt, rid, perm, st, sid, srel) in enumerate(named):
        out[i] = (e.type_id(rt), e.relation_id(rt, perm), e.intern(rt, rid), e.type_id(st), e.relation_id(st, srel) if srel else aclgpu.NO_RELATION, e.intern(st, sid))
    return out


def explain_family(aclgpu, e, c, want):
    """a seeded sample of the items through explain_proof (every mode) and explain / explain_denial / explain_revoke: an item those three flag as not
    explainable lies on a member with `-`, `&` or `.all()` beneath -- none on a monotone seed --, every other answer goes through its checker"""
    from aclgpu.text import parse_relationship
    rng = random.Random(f"explain/{c.mode}/{c.seed}")
    rels, nonmono = want["rels"], nonmono_of(c.schema)
    assert c.mode != "monotone" or not nonmono
    granted = [q for q, w in zip(c.items, want["checks"]) if w == HAS]
    denied = [q for q, w in zip(c.items, want["checks"]) if w == NO]
    done = {"proof": 0, "witness": 0, "denial": 0, "revoke": 0, "unsupported": 0}
    chk = P.ProofChecker(c.schema, rels)
    for q in rng.sample(granted, min(8, len(granted))):
        p, er, fl, lines = e.explain_proof(*q)
        assert (p, er) == HAS and fl == (aclgpu.EXPLAIN_PROOF if (q[0], q[2]) in nonmono else aclgpu.EXPLAIN_WITNESS), (q, p, er, fl)
        try:
            chk.check(q, [parse_relationship(ln) for ln in lines if not ln.startswith("not ")], [parse_relationship(ln[4:]) for ln in lines if ln.startswith("not ")])
        except AssertionError as x:
            raise AssertionError(f"explain_proof {q}: {x}") from None
        done["proof"] += 1
    for q in rng.sample(granted, min(8, len(granted))):
        p, er, fl, lines = e.explain(*q)
        assert (p, er) == HAS, (q, p, er)
        if fl == aclgpu.EXPLAIN_UNSUPPORTED:
            assert (q[0], q[2]) in nonmono and not lines, f"explain {q}: flagged unsupported on a monotone member"
            done["unsupported"] += 1
            continue
        assert fl == aclgpu.EXPLAIN_WITNESS and (q[0], q[2]) not in nonmono, (q, fl)
        try:
            X.check_witness(c.schema, set(rels), q, [parse_relationship(ln) for ln in lines])
        except AssertionError as x:
            raise AssertionError(f"explain {q}: {x}") from None
        done["witness"] += 1
    sample = rng.sample(denied, min(4, len(denied)))
    if sample:
        orcs = D.Oracles(c.schema, rels)
        perm, err, flags, off, recs = e.explain_denial_ids(item_ids(aclgpu, e, sample))
        for k, q in enumerate(sample):
            assert (int(perm[k]), int(err[k])) == NO, (q, int(perm[k]), int(err[k]))
            if int(flags[k]) == aclgpu.EXPLAIN_UNSUPPORTED:
                assert (q[0], q[2]) in nonmono and off[k] == off[k + 1], f"explain_denial {q}: flagged unsupported on a monotone member"
                done["unsupported"] += 1
                continue
            assert int(flags[k]) == aclgpu.EXPLAIN_DENIAL and (q[0], q[2]) not in nonmono, (q, int(flags[k]))
            try:
                D.check_grants(orcs, q, D.name_grants(e, c.schema, recs[off[k]:off[k + 1]]), seed=c.seed)
            except AssertionError as x:
                raise AssertionError(f"explain_denial {q}: {x}") from None
            done["denial"] += 1
    ck = R.Checker(c.schema, rels)
    for q in rng.sample(granted, min(4, len(granted))):
        p, er, fl, lines = e.explain_revoke(*q)
        assert (p, er) == HAS, (q, p, er)
        if fl == aclgpu.EXPLAIN_UNSUPPORTED:
            assert (q[0], q[2]) in nonmono and not lines, f"explain_revoke {q}: flagged unsupported on a monotone member"
            done["unsupported"] += 1
            continue
        assert fl == aclgpu.EXPLAIN_REVOKE and (q[0], q[2]) not in nonmono, (q, fl)
        try:
            ck.check(q, [parse_relationship(ln) for ln in lines])
        except AssertionError as x:
            raise AssertionError(f"explain_revoke {q}: {x}") from None
        done["revoke"] += 1
    return done


@pytest.mark.parametrize("mode,seed", params(SMALL))
def test_random_schema(mode, seed, aclgpu, monkeypatch):
    c = case_of(mode, seed)
    want = expected(mode, seed, 0)
    e = open_engine(aclgpu, c, c.rels)
    monkeypatch.setenv("ACL_LOCAL_MAX", "0")  # (read when an engine opens: the second one answers every Check by the level loop)
    lv = open_engine(aclgpu, c, c.rels)
    try:
        compare_reads(aclgpu, e, c, want, "walk", checks_only=True)
        st = e.stats()  # (after the one call of all items: which route answered THEM; a plain hand-over to the level loop moves no counter but expand_launches)
        route = "handed over to the level loop" if st["local_passes"] == 0 or st["expand_launches"] > 0 else "answered by the walk"
        # ... and the same items again, one call per object: a call whose walk overflows is redone as a whole by the level loop, so the walk's own
        # answers on a schema that fills a block's nodes are only ever compared in calls small enough for it.  At least one such call per seed is
        # answered by the walk alone.
        walked = calls = 0
        for k in range(0, len(c.items), len(c.subjects)):
            if k and c.items[k][:2] == c.items[k - 1][:2]:
                continue
            batch = [i for i, q in enumerate(c.items) if q[:2] == c.items[k][:2]]
            before = e.stats()
            perms, errs = e.check_bulk([c.items[i] for i in batch])
            after = e.stats()
            got = list(zip((int(p) for p in perms), (int(x) for x in errs)))
            assert got == [want["checks"][i] for i in batch], f"walk, the items of {c.items[k][:2]} alone"
            calls += 1
            walked += after["local_passes"] > before["local_passes"] and after["expand_launches"] == before["expand_launches"]
        # (a branching cycle, which half of the seeds may hold through monotone members, overflows the walk of every object that reaches it: the
        #  hand-over the issue calls legitimate -- such a seed may have no object left for the walk)
        from oracle.pyoracle import parse_schema
        branching = G.branching_cycle(parse_schema(c.schema), c.rels, monotone_too=True) is not None
        assert walked > 0 or branching, f"none of the {calls} per-object calls was answered by the single-launch walk"
        compare_reads(aclgpu, e, c, want, "walk")
        sa = e.stats()
        assert sa["local_passes"] > 0 or sa["overflow_retries"] > 0
        compare_reads(aclgpu, lv, c, want, "level loop", checks_only=True)
        sl = lv.stats()
        assert sl["local_passes"] == 0 and sl["expand_launches"] > 0
        done = explain_family(aclgpu, e, c, want)
        for n, (deletes, touches) in enumerate(c.rounds, 1):
            ups = [(aclgpu.OP_DELETE, r) for r in deletes] + [(aclgpu.OP_TOUCH, r) for r in touches]
            e.write(ups)
            lv.write(ups)
            compare_reads(aclgpu, e, c, expected(mode, seed, n), f"walk, after write round {n}")
            compare_reads(aclgpu, lv, c, expected(mode, seed, n), f"level loop, after write round {n}", checks_only=True)
        print(f"random schema {mode}-{seed}: {len(c.items)} items x 4 rounds x 2 routes, {route} (local_passes {st['local_passes']}, overflow_retries "
              f"{st['overflow_retries']}, expand_launches {st['expand_launches']}), {walked} of {calls} per-object calls by the walk alone, snapshot_patches {e.stats()['snapshot_patches']}, explained {done}")
    finally:
        e.close()
        lv.close()


def test_write_rounds_are_patched(aclgpu):
    """the write rounds reach the device as patches of the snapshot, not as rebuilds: over the corpus `snapshot_patches` rises (here: on its first seed)"""
    c = case_of(*SMALL[0])
    with open_engine(aclgpu, c, c.rels) as e:
        e.check_bulk(c.items[:8])
        before = e.stats()["snapshot_patches"]
        for deletes, touches in c.rounds:
            e.write([(aclgpu.OP_DELETE, r) for r in deletes] + [(aclgpu.OP_TOUCH, r) for r in touches])
            e.check_bulk(c.items[:8])
        assert e.stats()["snapshot_patches"] > before


@pytest.mark.parametrize("mode,seed", params(WIDE))
def test_wide_schema(mode, seed, aclgpu, monkeypatch):
    """40 objects per type and 100 users, the C oracle alone: Check on both routes, LookupResources, and the LookupSubjects rows of four resources per
    (type, permission) against a brute-force Check of every user -- on the targets where that brute force meets neither a depth error nor a wildcard"""
    c = case_of(mode, seed)
    co, _ = load_oracles(c.schema, c.rels, python=False)
    want = [co.check(*q) for q in c.items]
    e = open_engine(aclgpu, c, c.rels)
    monkeypatch.setenv("ACL_LOCAL_MAX", "0")
    lv = open_engine(aclgpu, c, c.rels)
    try:
        for where, eng in (("walk", e), ("level loop", lv)):
            perms, errs = eng.check_bulk(c.items)
            got = list(zip((int(p) for p in perms), (int(x) for x in errs)))
            bad = [(q, g, w) for q, g, w in zip(c.items, got, want) if g != w]
            assert not bad, f"{where}: {len(bad)} Checks differ (item, engine, C oracle): {bad[:4]}"
        sl = lv.stats()
        assert sl["local_passes"] == 0 and sl["expand_launches"] > 0
        for t in c.lookup_targets:
            g, w = outcome(e.lookup, *t), outcome(co.lookup, *t)
            assert g == w, f"LookupResources {t}: engine {g}, C oracle {w}"
        rows = 0
        people = c.types["user"]  # (the user no relationship names among them: whoever grants it is a wildcard)
        for k, (t, ms) in enumerate(c.members.items()):
            for j, m in enumerate(ms):
                if m not in G.PERM_NAMES:
                    continue
                for rid in c.types[t][(7 * k + 3 * j) % 10::10]:
                    ans = {u: co.check(t, rid, m, "user", u) for u in people}
                    if any(err for _, err in ans.values()) or ans[G.NOBODY] == HAS:
                        continue
                    names, wild, excluded = e.lookup_subjects(t, rid, m, "user")
                    assert (names, wild, excluded) == ({u for u, a in ans.items() if a == HAS}, False, set()), (t, rid, m)
                    rows += 1
        assert rows > 0
        st = e.stats()  # (read where test_random_schema reads them: after every read of the default engine)
        assert st["local_passes"] > 0 or st["overflow_retries"] > 0
        print(f"random schema {mode}-{seed}: {len(c.items)} items x 2 routes, {len(c.lookup_targets)} lookups, {rows} LookupSubjects rows; local_passes "
              f"{st['local_passes']}, overflow_retries {st['overflow_retries']}, expand_launches {st['expand_launches']}")
    finally:
        e.close()
        lv.close()


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("mode,seed", SHARDED, ids=[f"{m}-{s}" for m, s in SHARDED])
def test_sharded(mode, seed, world, aclgpu):
    """the same schemas on `world` logical shards of one device, through the native level loops: every rank's Check, LookupResources and LookupSubjects
    equal the oracles' answers test_random_schema holds the single engine to"""
    from tests.test_sharded_subjects_gpu import run_shards
    c = case_of(mode, seed)
    want = expected(mode, seed, 0)
    assert all(cw == pw for _t, cw, pw in want["lookups"])
    lookups = [(t, cw) for t, cw, _pw in want["lookups"]][::2]
    subjects = want["subjects"][::3]

    def load(e):
        for k in range(0, len(c.rels), 500):
            e.write([(aclgpu.OP_TOUCH, r) for r in c.rels[k:k + 500]])
        for t, objs in c.types.items():
            for o in objs:
                e.intern(t, o)

    def fn(se):
        e = se.shard.e
        perm, err, _ = se.check_bulk_ids_native(item_ids(aclgpu, e, c.items))
        checks = list(zip(perm.cpu().numpy().tolist(), err.cpu().numpy().tolist()))
        got_l, got_s = [], []
        for (rt, m, st, sid, srel), _w in lookups:
            try:
                bm, _ = se.lookup_ids_batch_native(rt, m, st, srel, [e.intern(st, sid)])
                got_l.append(("ok", set(e.bitmap_names(rt, bm[0].cpu().numpy().view(np.uint32)))))
            except aclgpu.AclError as x:
                got_l.append(("err", x.code))
        for (rt, m, rid, st, srel), _w in subjects:
            try:
                bm, flags, ex, _ = se.lookup_subjects_ids_batch_native(rt, m, st, srel, [e.intern(rt, rid)], want_excluded=True)
                wild = bool(flags[0] & 1)
                got_s.append((set(e.bitmap_names(st, bm[0].cpu().numpy().view(np.uint32))), wild,
                              set(e.bitmap_names(st, ex[0].cpu().numpy().view(np.uint32))) if wild else set()))
            except aclgpu.AclError as x:
                if x.code != aclgpu.ERR_DEPTH:
                    raise
                got_s.append("DEPTH")
        return checks, got_l, got_s

    for rank, (checks, got_l, got_s) in enumerate(run_shards(aclgpu, world, c.schema, load, fn)):
        bad = [(q, g, w) for q, g, w in zip(c.items, checks, want["checks"]) if tuple(g) != w]
        assert not bad, f"rank {rank}: {len(bad)} Checks differ (item, engine, oracles): {bad[:4]}"
        for (t, w), g in zip(lookups, got_l):
            assert g == w, f"rank {rank}: LookupResources {t}: engine {g}, oracles {w}"
        for (t, w), g in zip(subjects, got_s):
            assert g == w, f"rank {rank}: LookupSubjects {t}: engine {g}, contract {w}"

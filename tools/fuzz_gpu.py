#!/usr/bin/env python3
"""usage (GPU box): tools/fuzz_gpu.py [--seed S] [--steps N] -- differential fuzz of the engine against the CPU oracle on a LIVE graph.

A nested-group / arrow graph (the C4 schema, cycles allowed) is mutated step by step -- TOUCH / CREATE / DELETE batches, filter deletes --
and between the writes both sides answer the same random Check batches (1 ... 70 000 items: the single-launch walk's 4-wave and 16-wave
kernels, the host-mapped small-batch path, the micro-batcher's single checks) and LookupResources requests (single and batched).  Every
answer, every error code and every allowed-id set must be equal.  Writes land in the device snapshot as in-place patches, background
compactions happen when the headroom runs low: the fuzz is what exercises patch -> query -> patch sequences nobody wrote a test for.
The oracle is the checker (tests / tools only).  Exit code 1 and a dump of the first difference on a mismatch.

--reads (run_reads) is the same kind of write stream under the engine's other read paths, each held to the oracles between the writes:
  a. LookupSubjects -- batches of 1, 5 and 33 resources, the n = 1 call, the string form, a group#member subject form -- against the C oracle's Check (C4
     schema) or the contract of tests/subjects_contract.py (combine schema: ids, wildcard, excluded, or the call fails at the depth limit);
  b. Explain witness: perm / err of the oracle's Check, a witness for every item a monotone permission grants, each through tests/explain_checker.py;
  c. Explain proof (combine schema): every granted item proved, each proof through tests/proof_checker.py;
  d. Explain denial (monotone permissions): the grants through tests/denial_checker.py;
  e. multi-target LookupResources over every relation and permission, bit for bit the single-target rows, by name the oracle's lookups, and access_review;
  f. lookup, subject and mixed cursors held open across later writes, compactions and recycled ids, with derived cursors and counts over them.
--reads --dry is the oracle's half alone (no GPU).  --expiry also asks LookupSubjects and Explain about live and expired idempotency keys.

  g. Explain for revocation: the cut set of granted monotone items against the brute force over the relationships, each through tests/revoke_checker.py;
  h. (--expiring) a resource-direction and a subject-direction watch set on pod#view, polled against the difference of the oracle's rows since the last poll.

--expiring (run, run_reads, run_patcher, run_sharded; with --dry too) is each campaign on the schema's expiring variant (SCHEMA_C4_EXPIRING / SCHEMA_COMBINE_EXPIRING:
`with expiration` on every relation but the creators and pod#auditor) under a test clock (class Clock).  Both sides start at 1 700 000 000; two TOUCH / CREATE
updates in five carry an expiry (now + 1 s ... 200 000 s, now and then now - 5: born expired; on a relation without the trait both sides must refuse the request
with the same code); one step in four is a clock move in place of a write -- forward by 1 s ... 90 000 s, one time in five BACK by 1 ... 4 000 s.  The backward
rule: the oracles do not model the collection of relationships that expired 24 h ago (Store::gc_expired, inside the next write), so one the store has collected
would come back to life in the oracle if the clock fell below its expiry; the clock therefore never goes more than 6 h below the highest value it has had, which
keeps every collected relationship expired on both sides.  Around every move the oracle answers a fixed probe batch of Check items before and after, the engine
after; the oracle's read difference across the move says what ran out (nestings, tuplesets, bans, wildcards).  The pool that deletes draw from is read back from
the oracle behind every move and every accepted write.  Without --expiring every stream is draw for draw what it was.

--sharded W (run_sharded) holds the loops of the type-hash sharded graph to the oracles under the same kind of stream.  Phase 1, no GPU: one pass with the oracles
alone writes the script -- every write with its outcome, every read with its expected answer by name.  Phase 2: W logical shards of one GPU (one engine per rank over
a replicated store, one thread each) replay it; a rank records a wrong answer as (step, rank, kind, request, got, want) and goes on, the first record is printed:
  a. Check batches of 1, 7, 64, 900, 3000 items through acl_shard_check_bulk and, on the same step, the host-driven step protocol (--exchange), route against route;
  b. LookupResources of 1 and 4 subjects through acl_shard_lookup_bulk and the host-driven protocol, or the oracle's failure code on every rank and a correct next call;
  c. LookupSubjects of 1, 5, 33 resources with excluded rows through acl_shard_subjects_bulk, user and group#member subjects, or ACL_ERR_DEPTH on every rank;
  d. levels / retries / entries_exchanged / host_syncs / export_capacity of every native call (burst hints outrun by a deeper batch, grow-and-redo under --xcap).
On --schema combine the host-driven protocol refuses the schema (its code is recorded once) and the native loops alone answer.  --sharded W --dry is phase 1 plus the
script's writes on W store-only engines (acl_shard_configure) whose patched host snapshot is verified against the store at every read step."""
import argparse
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "spicedb-kubeapi-proxy_amd")]


# The C4 schema with every non-monotone construct the engine compiles into combine programs (plan.hpp BX_*): exclusion at the top of a permission
# that arrows reach, intersection over an arrow, a userset subject that is itself a non-monotone permission (group#active), wildcards on both
# sides of a `-`, and a permission that subtracts an intersection.  Cycles through group#member (and through group#active, via pod viewers) stay
# legal: a non-monotone cycle ends at the depth limit on both sides.  `everywhere` / `vetted`: intersection arrows over a pod's namespaces (a
# fifth of the pod#namespace relationships name a second namespace).
SCHEMA_COMBINE = """
definition user {}
definition group {
  relation member: user | group#member
  relation banned: user
  permission active = member - banned
}
definition namespace {
  relation viewer: user | group#member | user:*
  relation creator: user
  relation banned: user | group#member
  permission view = (viewer + creator) - banned
}
definition pod {
  relation namespace: namespace
  relation viewer: user | group#member | group#active
  relation creator: user
  relation auditor: user | group#member
  relation banned: user | user:*
  permission view = (viewer + creator + namespace->view) - banned
  permission audit = auditor & namespace->view
  permission edit = creator + (viewer & auditor) - banned
  permission hidden = view - (auditor & creator)
  permission everywhere = namespace.all(view)
  permission vetted = creator + namespace.all(view) & viewer
}
"""


# The two schemas with `with expiration` on every alternative of group#member, namespace#viewer, namespace#banned, pod#namespace, pod#viewer, pod#banned and
# group#banned (run(expiring=True) and its kin); pod#creator, namespace#creator and pod#auditor stay without the trait: a write that gives one of them an
# expiry is refused, by the engine and by the oracle with the same code.
SCHEMA_C4_EXPIRING = """
definition user {}
definition group {
  relation member: user with expiration | group#member with expiration
}
definition namespace {
  relation viewer: user with expiration | group#member with expiration
  relation creator: user
  permission view = viewer + creator
}
definition pod {
  relation namespace: namespace with expiration
  relation viewer: user with expiration | group#member with expiration
  relation creator: user
  permission view = viewer + creator + namespace->view
}
"""

SCHEMA_COMBINE_EXPIRING = """
definition user {}
definition group {
  relation member: user with expiration | group#member with expiration
  relation banned: user with expiration
  permission active = member - banned
}
definition namespace {
  relation viewer: user with expiration | group#member with expiration | user:* with expiration
  relation creator: user
  relation banned: user with expiration | group#member with expiration
  permission view = (viewer + creator) - banned
}
definition pod {
  relation namespace: namespace with expiration
  relation viewer: user with expiration | group#member with expiration | group#active with expiration
  relation creator: user
  relation auditor: user | group#member
  relation banned: user with expiration | user:* with expiration
  permission view = (viewer + creator + namespace->view) - banned
  permission audit = auditor & namespace->view
  permission edit = creator + (viewer & auditor) - banned
  permission hidden = view - (auditor & creator)
  permission everywhere = namespace.all(view)
  permission vetted = creator + namespace.all(view) & viewer
}
"""

CLOCK_START = 1_700_000_000
CLOCK_BACK_LIMIT = 6 * 3600   # a clock set back stays within 6 h of the highest value it has had (see Clock)
COLLECT_AFTER = 86400         # Store::gc_expired: a relationship expired this long is collected inside the next write
CLOCK_STATS = ("clock_forward", "clock_back", "lost_by_clock", "gained_by_clock", "gained_by_clock_back", "expired_nestings", "expired_tuplesets", "expired_bans",
               "expired_wildcards", "collected_due", "writes_with_expiry", "expiry_refused")


def schema_text_of(schema: str, expiring: bool = False) -> str:
    from aclgpu import workloads
    if schema == "combine":
        return SCHEMA_COMBINE_EXPIRING if expiring else SCHEMA_COMBINE
    return SCHEMA_C4_EXPIRING if expiring else workloads.SCHEMA_C4


def read_live(o) -> set:
    """the relationships the oracle reads at its clock, as texts"""
    return set(f"{a}:{b}#{c}@{d}:{x}" + (f"#{y}" if y else "") for t in ("group", "namespace", "pod") for a, b, c, d, x, y, *_ in o.read(rtype=t))


class Clock:
    """The test clock of an expiring run: both sides start at CLOCK_START, every draw comes from the write stream's generator (and only when the run is an
    expiring one, so every other case's stream stays draw for draw what it was).
      * write_batch gives a TOUCH / CREATE an expiry with probability 0.4: now + 1 s ... 200 000 s, one time in ten now - 5 (born expired).  On a relation
        without the trait (the creators, pod#auditor) about one such write in seven keeps the expiry: both sides must refuse the request with the same code.
      * move(): forward by 1 s ... 90 000 s, one time in five BACK by 1 ... 4 000 s.  The oracles do not model the collection of relationships that expired 24 h
        ago (Store::gc_expired, inside the next write): one the store has collected would come back to life in the oracle if the clock fell below its expiry.  So
        the clock never goes more than 6 h below the highest value it has had -- every collected relationship stays expired on both sides.
    around(): the probe batch (about 200 Check items, chosen once per run from a generator of their own) is answered by the oracle before and after a move and by
    the engines after it; the answers and the oracle's read difference across the move feed the CLOCK_STATS counters.  The batch is chosen at the first move:
    random Check items, half of them granted on the graph of that moment (most random items are denied whatever the clock says)."""

    def __init__(self, rng, seed, names, combine, o, engines, stats, probe: int = 200):
        self.rng, self.o, self.engines, self.stats, self.combine = rng, o, [e for e in engines if e is not None], stats, combine
        self.now = self.high = CLOCK_START
        self.expiries = {}      # relationship text -> expiry, of the accepted writes that carried one and are neither deleted nor rewritten nor counted as collected
        self.moved_last = False  # the step before was a clock move (no accepted write since)
        self.probe, self._probe_of = None, (random.Random(f"probe/{seed}"), names, probe)
        for k in CLOCK_STATS:
            stats.setdefault(k, 0)
        for x in [o] + self.engines:
            x.set_now(self.now)

    def expiry_for(self, text, refusable=True):
        """the expiry a TOUCH / CREATE of `text` carries (0: none); refusable: a relation without the trait may keep it"""
        rng = self.rng
        if rng.random() >= 0.4:
            return 0
        at = self.now - 5 if rng.random() < 0.1 else self.now + rng.choice([1, 5, 60, 3600, 86400, 200000])
        rel = text.split("#", 1)[1].split("@", 1)[0]
        if rel in ("creator", "auditor") and (not refusable or rng.random() >= 0.15):
            return 0
        return at

    def accepted(self, ups, delete_op):
        """an accepted write batch: what it leaves with an expiry, and how many relationships expired for 24 h the store collects inside it"""
        for u in ups:
            self.expiries.pop(u[1], None)
            if u[0] != delete_op and len(u) > 2 and u[2]:
                self.expiries[u[1]] = u[2]
        due = [t for t, at in self.expiries.items() if at <= self.now - COLLECT_AFTER]
        for t in due:
            del self.expiries[t]
        self.stats["collected_due"] += len(due)
        self.moved_last = False

    def filtered(self, f):
        """an accepted DeleteRelationships by filter `f`: what it removed is not there to collect"""
        from oracle import orc
        keys = ("rtype", "rid", "rel", "stype", "sid", "srel")
        for t in [t for t in self.expiries if all(f.get(k) is None or f[k] == v for k, v in zip(keys, orc.parse_rel(t)))]:
            del self.expiries[t]
        self.moved_last = False

    def draw_move(self) -> int:
        rng = self.rng
        if rng.random() < 0.2:
            d = -rng.choice([1, 20, 200, 4000])
            return max(d, self.high - CLOCK_BACK_LIMIT - self.now)
        return rng.choice([1, 1, 3, 10, 61, 3601, 50000, 90000])

    def move(self, step, live=None, check=None):
        """one clock step on every side -> (delta, relationships the oracle read before and not after, probe answers after).  check(probe, want, where): how
        the caller's engine answers the probe batch (None: the oracle alone)."""
        o, st = self.o, self.stats
        d = self.draw_move()
        if self.probe is None:
            pr, names, n = self._probe_of
            has, rest = [], []
            for q in dict.fromkeys(rand_query(pr, names, self.combine) for _ in range(20 * n)):
                side = has if tuple(o.check(*q)) == (2, 0) else rest
                if len(side) < n // 2:
                    side.append(q)
            self.probe = has + rest
        before = read_live(o)
        was = [tuple(o.check(*q)) for q in self.probe]
        self.now += d
        self.high = max(self.high, self.now)
        for x in [o] + self.engines:
            x.set_now(self.now)
        after = read_live(o)
        want = [tuple(o.check(*q)) for q in self.probe]
        st["clock_forward" if d > 0 else "clock_back"] += d != 0
        lost = sum(a == (2, 0) and b != (2, 0) for a, b in zip(was, want))
        gained = sum(a != (2, 0) and b == (2, 0) for a, b in zip(was, want))
        st["lost_by_clock"] += lost
        st["gained_by_clock" if d > 0 else "gained_by_clock_back"] += gained
        for t in before - after:
            head, subj = t.split("@", 1)
            st["expired_nestings"] += head.startswith("group:") and head.endswith("#member") and subj.startswith("group:")
            st["expired_tuplesets"] += head.endswith("#namespace")
            st["expired_bans"] += head.endswith("#banned")
            st["expired_wildcards"] += subj.endswith(":*")
        if live is not None:
            live.clear()
            live.update(after)
        self.moved_last = True
        if check is not None:
            check(self.probe, want, f"step {step} (clock {'+' if d > 0 else ''}{d} s, now {self.now})")
        return d, before - after, want


def make_universe(rng, universe: int = 1):
    """(users, groups, namespaces, pods): the names the write stream draws from.  The pods' namespaces are the stream's first draws from `rng`."""
    users = [f"u{i}" for i in range(160 * universe)]
    groups = [f"g{i}" for i in range(48 * universe)]
    nss = [f"n{i}" for i in range(8 * universe)]
    pods = [f"{rng.choice(nss)}/p{i}" for i in range(240 * universe)]
    return users, groups, nss, pods


def make_rand_tuple(rng, names, combine: bool = False, recycle: bool = False, acyclic: bool = False):
    """-> rand_tuple(): one random relationship text over `names` (make_universe), every draw from `rng`; rand_tuple.fresh[0] counts the never-seen names"""
    users, groups, nss, pods = names
    fresh = [0]

    def rand_tuple():
        if recycle and rng.random() < 0.15:  # objects nobody has named before: they take over the ids of objects that lost their last relationship
            fresh[0] += 1
            return rng.choice([f"pod:{rng.choice(nss)}/fresh{fresh[0]}#viewer@user:{rng.choice(users)}", f"pod:{rng.choice(pods)}#viewer@user:newcomer{fresh[0]}",
                               f"group:team{fresh[0]}#member@user:{rng.choice(users)}", f"pod:{rng.choice(pods)}#viewer@group:team{fresh[0] - rng.randrange(3)}#member"])
        if combine and rng.random() < 0.3:  # the relations only the combine schema has
            k = rng.randrange(9)
            if k == 0: return f"group:{rng.choice(groups)}#banned@user:{rng.choice(users)}"
            if k == 1: return f"namespace:{rng.choice(nss)}#banned@user:{rng.choice(users)}"
            if k == 2: return f"namespace:{rng.choice(nss)}#banned@group:{rng.choice(groups)}#member"
            if k == 3: return f"namespace:{rng.choice(nss)}#viewer@user:*" if rng.random() < 0.3 else f"pod:{rng.choice(pods)}#viewer@group:{rng.choice(groups)}#active"
            if k == 4: return f"pod:{rng.choice(pods)}#auditor@user:{rng.choice(users)}"
            if k == 5: return f"pod:{rng.choice(pods)}#auditor@group:{rng.choice(groups)}#member"
            if k == 6: return f"pod:{rng.choice(pods)}#banned@user:{rng.choice(users)}"
            if k == 7: return f"pod:{rng.choice(pods)}#banned@user:*" if rng.random() < 0.2 else f"pod:{rng.choice(pods)}#banned@user:{rng.choice(users)}"
            return f"pod:{rng.choice(pods)}#viewer@group:{rng.choice(groups)}#active"
        k = rng.randrange(9)
        if k == 0 and acyclic:  # (--acyclic: a group only holds groups behind it in the list -- no Check ends at the depth limit, one-user calls take the reverse walk)
            i, j = sorted(rng.sample(range(len(groups)), 2))
            return f"group:{groups[i]}#member@group:{groups[j]}#member"
        if k == 0: return f"group:{rng.choice(groups)}#member@group:{rng.choice(groups)}#member"   # (cycles welcome)
        if k == 1: return f"group:{rng.choice(groups)}#member@user:{rng.choice(users)}"
        if k == 2: return f"pod:{(p := rng.choice(pods))}#namespace@namespace:{p.split('/')[0] if rng.random() < 0.8 else rng.choice(nss)}"
        if k == 3: return f"pod:{rng.choice(pods)}#creator@user:{rng.choice(users)}"
        if k == 4: return f"namespace:{rng.choice(nss)}#creator@user:{rng.choice(users)}"
        if k == 5: return f"pod:{rng.choice(pods)}#viewer@user:{rng.choice(users)}"
        if k == 6: return f"pod:{rng.choice(pods)}#viewer@group:{rng.choice(groups)}#member"
        if k == 7: return f"namespace:{rng.choice(nss)}#viewer@user:{rng.choice(users)}"
        return f"namespace:{rng.choice(nss)}#viewer@group:{rng.choice(groups)}#member"

    rand_tuple.fresh = fresh
    return rand_tuple


def rand_query(rng, names, combine: bool = False):
    """one random Check item (rtype, rid, permission, stype, sid, srel) over `names`, every draw from `rng`"""
    users, groups, nss, pods = names
    k = rng.randrange(10)
    u = rng.choice(users) if rng.random() < 0.97 else "stranger"
    if combine and rng.random() < 0.45:
        kk = rng.randrange(6)
        if kk < 3: return ("pod", rng.choice(pods), rng.choice(("audit", "edit", "hidden", "everywhere", "vetted")), "user", u, "")
        if kk == 3: return ("group", rng.choice(groups), "active", "user", u, "")
        if kk == 4: return ("pod", rng.choice(pods), "view", "group", rng.choice(groups), "active")  # a non-monotone userset as the subject
        return ("namespace", rng.choice(nss), "view", "group", rng.choice(groups), "member")
    if k < 6: return ("pod", rng.choice(pods) if rng.random() < 0.97 else "n0/ghost", "view", "user", u, "")
    if k < 8: return ("namespace", rng.choice(nss), "view", "user", u, "")
    if k < 9: return ("group", rng.choice(groups), "member", "user", u, "")
    return ("pod", rng.choice(pods), "view", "group", rng.choice(groups), "member")  # a userset as the subject


def open_engine(schema_text: str, recycle: bool, compact_early: bool, **engine_kw):
    import aclgpu
    if recycle:
        os.environ["ACL_ID_QUARANTINE_MS"] = "0"  # (read when the schema is loaded) freed ids are reused by the next new name at once
    if compact_early:
        os.environ["ACL_COMPACTION_SLACK"] = "0"  # (read at acl_open) background compactions, adopted with the writes since replayed, on this small graph too
    try:
        return aclgpu.Engine(schema_text, **engine_kw)
    finally:
        os.environ.pop("ACL_COMPACTION_SLACK", None)
        os.environ.pop("ACL_ID_QUARANTINE_MS", None)


def load_initial(rand_tuple, o, e, live: set, universe: int = 1, clock=None):
    """the starting graph: 2500 draws of rand_tuple per universe, written to the oracle and (unless e is None) to the engine; under a Clock two in five of its
    relationships carry an expiry where the relation has the trait"""
    import aclgpu
    from oracle import orc
    init = list(dict.fromkeys(rand_tuple() for _ in range(2500 * universe)))
    if clock is not None:
        init = [(t, clock.expiry_for(t, refusable=False)) for t in init]
        init = [(t, at) if at else (t,) for t, at in init]
    else:
        init = [(t,) for t in init]
    for i in range(0, len(init), 500):
        o.write([(orc.OP_TOUCH,) + u for u in init[i:i + 500]])
        if e is not None:
            e.write([(aclgpu.OP_TOUCH,) + u for u in init[i:i + 500]])
    if clock is not None:
        clock.accepted([(aclgpu.OP_TOUCH,) + u for u in init], aclgpu.OP_DELETE)
        live.update(read_live(o))
    else:
        live.update(u[0] for u in init)


def write_batch(rng, step, rand_tuple, o, e, live: set, burst: int, stats: dict, clock=None) -> bool:
    """One write batch (TOUCH / CREATE / DELETE) on both sides, which accept it or reject it with the same code; e is None: the oracle alone.
    clock: a Clock -- some TOUCH / CREATE updates carry an expiry (Clock.expiry_for), and `live` is read back from the oracle behind an accepted batch.
    -> True when it was accepted (`live` follows it)."""
    import aclgpu
    from oracle import orc
    ups = []
    pool = sorted(live) if live else []  # (once per batch: a delete picks from the relationships that exist)

    def upsert(op):
        t = rand_tuple()
        at = clock.expiry_for(t) if clock is not None else 0
        return (op, t, at) if at else (op, t)

    for _ in range(rng.randrange(1, burst)):
        q = rng.random()
        if q < 0.5: ups.append(upsert(aclgpu.OP_TOUCH))
        elif q < 0.5 + 0.1 / max(1, burst // 25): ups.append(upsert(aclgpu.OP_CREATE))
        elif pool: ups.append((aclgpu.OP_DELETE, rng.choice(pool) if rng.random() < 0.9 else rand_tuple()))
    ups = list({u[1]: u for u in ups}.values())  # one update per relationship in a request
    eo = ee = None
    try:
        o.write([({aclgpu.OP_TOUCH: orc.OP_TOUCH, aclgpu.OP_CREATE: orc.OP_CREATE, aclgpu.OP_DELETE: orc.OP_DELETE}[u[0]],) + tuple(u[1:]) for u in ups])
    except orc.OracleError as x:
        eo = x.code
    if e is not None:
        try:
            e.write(ups)
        except aclgpu.AclError as x:
            ee = x.code
        assert eo == ee, f"step {step}: write outcome differs: oracle {eo}, engine {ee}: {ups}"
    stats["writes"] += 1
    if clock is not None:
        stats["writes_with_expiry"] += any(len(u) > 2 for u in ups)
        stats["expiry_refused"] += eo is not None and any(len(u) > 2 and u[1].split("#", 1)[1].split("@", 1)[0] in ("creator", "auditor") for u in ups)
    if eo is None:
        for u in ups:
            (live.discard if u[0] == aclgpu.OP_DELETE else live.add)(u[1])
        if clock is not None:  # (a relationship born expired is not there to delete: the pool is what the oracle reads)
            clock.accepted(ups, aclgpu.OP_DELETE)
            live.clear()
            live.update(read_live(o))
    else:
        stats["write_errors"] += 1
    return eo is None


def filter_delete(rng, step, names, combine: bool, o, e, live: set, stats: dict, clock=None) -> int:
    """DeleteRelationships by one random filter on both sides (e is None: the oracle alone) -> how many relationships it removed; `live` is read back"""
    users, groups, nss, pods = names
    f = rng.choice([dict(rtype="pod", rid=rng.choice(pods)), dict(rtype="group", rel="member", stype="user", sid=rng.choice(users)),
                    dict(rtype="namespace", rid=rng.choice(nss), rel="viewer")] +
                   ([dict(rtype="pod", rel="banned", stype="user", sid="*"), dict(rtype="namespace", rel="banned")] if combine else []))
    n1 = o.delete_by_filter(**f)
    if e is not None:
        n2 = e.delete_by_filter(**f)
        assert n1 == n2, f"step {step}: delete_by_filter {f}: oracle removed {n1}, engine {n2}"
    now = read_live(o)
    live.clear()
    live.update(now)
    stats["filter_deletes"] += 1
    if clock is not None and n1:
        clock.filtered(f)
    return n1


def run(seed: int, steps: int, big: int = 70000, verbose: bool = True, burst: int = 25, universe: int = 1, compact_early: bool = False, schema: str = "c4",
        recycle: bool = False, acyclic: bool = False, expiring: bool = False, engine: bool = True, probe: int = 200) -> dict:
    """The Check campaign (the header's first paragraph).  expiring: the schema's expiring variant under a Clock -- writes with an expiry, one step in four a
    clock move with the probe batch answered around it.  engine=False: the oracle's half alone (no GPU): what the stream covers."""
    from oracle import orc
    combine = schema == "combine"
    schema_text = schema_text_of(schema, expiring)

    rng = random.Random(seed)
    names = users, groups, nss, pods = make_universe(rng, universe)
    rand_tuple = make_rand_tuple(rng, names, combine, recycle, acyclic)

    e = open_engine(schema_text, recycle, compact_early) if engine else None
    o = orc.Oracle(schema_text)
    live = set()
    stats = {"writes": 0, "write_errors": 0, "filter_deletes": 0, "checks": 0, "lookups": 0, "single_checks": 0}
    clock = Clock(rng, seed, names, combine, o, [e], stats, probe) if expiring else None  # (before the first write: the starting graph is written at the clock's start)
    load_initial(rand_tuple, o, e, live, universe, clock)
    if e is not None:
        e.batcher_start(4096, 100)

    def probe_check(qs, want, where):
        perms, errs = e.check_bulk(qs)
        for i, q in enumerate(qs):
            assert (perms[i], errs[i]) == want[i], f"{where}: probe check {q} (item {i}): engine {(perms[i], errs[i])}, oracle {want[i]}"
        stats["checks"] += len(qs)

    t0 = time.time()
    for step in range(steps):
        if clock is not None and rng.random() < 0.25:  # ---- the clock moves: no write, and the next read sees every relationship whose liveness changed
            clock.move(step, live, probe_check if e is not None else None)
            continue
        r = rng.random()
        if r < 0.45:  # ---- a write batch: both sides accept it or reject it with the same code
            write_batch(rng, step, rand_tuple, o, e, live, burst, stats, clock)
        elif r < 0.5:  # ---- DeleteRelationships by filter
            filter_delete(rng, step, names, combine, o, e, live, stats, clock)
        elif r < 0.56 and not combine:  # ---- PostFilter's shape: ONE user's pairs -- CheckBulkPermissions itself twice (the second call may sweep the type for depth
            # errors and take the reverse walk: engine_keep.cpp no_object_is_deep; with a cycle behind some resource the calls stay forward and carry its depth errors),
            # then the keep mask of the same pairs.  Every permissionship, every error and every keep byte against the oracle.
            rt, perm, ids = rng.choice([("pod", "view", pods), ("namespace", "view", nss), ("group", "member", groups)])
            u = rng.choice(users) if rng.random() < 0.9 else "stranger"
            k_ = rng.choice([520, 900, 2500])
            qs = [(rt, rng.choice(ids) if rng.random() < 0.98 else "n0/ghost", perm, "user", u, "") for _ in range(k_)]
            want = {q: o.check(*q) for q in set(qs)}
            for rep in range(2 if e is not None else 0):
                perms, errs = e.check_bulk(qs)
                for i, q in enumerate(qs):
                    assert (perms[i], errs[i]) == tuple(want[q]), f"step {step}: one-user check {q} (item {i} of {k_}, call {rep}): engine {(perms[i], errs[i])}, oracle {want[q]}"
            keep = e.check_bulk_keep(qs, list(range(k_ + 1))) if e is not None else []
            for i, q in enumerate(qs[:len(keep)]):
                assert bool(keep[i]) == (tuple(want[q]) == (2, 0)), f"step {step}: keep mask of {q} (item {i}): engine {keep[i]}, oracle {want[q]}"
            stats["checks"] += 3 * k_
            stats["one_user_calls"] = stats.get("one_user_calls", 0) + 3
        elif r < 0.85:  # ---- a Check batch
            n = rng.choice([1, 1, 7, 64, 64, 900, 5000, big if step % 7 == 3 else 3000])
            qs = [rand_query(rng, names, combine) for _ in range(min(n, 6000))]
            qs = (qs * (n // len(qs) + 1))[:n]
            want = {q: o.check(*q) for q in set(qs)}
            if n == 1 and rng.random() < 0.5:  # the micro-batcher's single check
                got = [e.check_one(*qs[0])] if e is not None else []
                stats["single_checks"] += 1
            elif e is not None:
                perms, errs = e.check_bulk(qs)
                got = list(zip(perms, errs))
            else:
                got = []
            for i, q in enumerate(qs[:len(got)]):
                assert tuple(got[i]) == tuple(want[q]), f"step {step}: check {q} (item {i} of {n}): engine {got[i]}, oracle {want[q]}"
            stats["checks"] += n
        else:  # ---- LookupResources: one subject, or a batch of subjects in one walk
            rt, perm = rng.choice([("pod", "view"), ("namespace", "view"), ("group", "member")] +
                                  ([("pod", "audit"), ("pod", "edit"), ("pod", "hidden"), ("group", "active"), ("pod", "everywhere"), ("pod", "vetted")] if combine else []))
            subs = rng.sample(users, rng.choice([1, 1, 3, 20]))
            def out(fn, *a):  # ("ok", ids) or ("err", code): a lookup whose candidate's Check errs fails as a whole, in the engine and in the oracle
                try:
                    return ("ok", sorted(fn(*a)))
                except Exception as ex:  # noqa: BLE001
                    if getattr(ex, "code", None) is None:
                        raise
                    return ("err", ex.code)

            for u in subs[:3]:
                b = out(o.lookup, rt, perm, "user", u)
                a = out(e.lookup, rt, perm, "user", u) if e is not None else b
                assert a == b, f"step {step}: lookup {rt}#{perm}@user:{u}: engine {a[0]} {str(a[1])[:200]}, oracle {b[0]} {str(b[1])[:200]}"
                stats["lookups_failed"] = stats.get("lookups_failed", 0) + int(a[0] == "err")
            if len(subs) > 3:
                wants = [out(o.lookup, rt, perm, "user", u) for u in subs]
            if len(subs) > 3 and e is not None:
                ids = [e.intern("user", u) for u in subs]
                batch = out(lambda: [0] if e.lookup_ids_batch(rt, perm, "user", "", ids) is None else [1])
                if any(w_[0] == "err" for w_ in wants):  # one failing lookup fails the batch call
                    assert batch[0] == "err", f"step {step}: batched lookup {rt}#{perm}: the oracle fails {[u for u, w_ in zip(subs, wants) if w_[0] == 'err'][:3]}, the engine answered"
                else:
                    bm, counts = e.lookup_ids_batch(rt, perm, "user", "", ids)
                    for j, u in enumerate(subs):
                        got = sorted(e.object_name(rt, i) for i in range(e.object_count(rt)) if (bm[j][i >> 5] >> (i & 31)) & 1)
                        assert got == wants[j][1], f"step {step}: batched lookup {rt}#{perm}@user:{u}"
            stats["lookups"] += len(subs)
        if verbose and step % 50 == 49:
            print(f"step {step + 1}/{steps}: {stats}, {len(live)} relationships, {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
    stats["seconds"] = round(time.time() - t0, 1)
    if e is not None:
        st = e.stats()
        stats.update({k: int(st[k]) for k in ("snapshot_builds", "snapshot_patches", "snapshot_compactions", "local_passes", "rev_local_passes", "ids_recycled", "keep_route_calls", "depth_sweeps") if k in st})
        e.close()
    return stats


def nonmono_members(defs) -> set:
    """{(type, member)}: the relations and permissions with `-`, `&` or `.all()` anywhere beneath (a least fixpoint over references, arrows and userset subjects)"""
    from oracle.pyoracle import Relation
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
                if (t, m) in nm:
                    continue
                if any(a[1] and a[1] != "*" and (a[0], a[1]) in nm for a in mem.allowed) if isinstance(mem, Relation) else expr(t, mem.expr):
                    nm.add((t, m))
                    changed = True
    return nm


def _ids_of(row):
    import numpy as np
    return np.flatnonzero(np.unpackbits(np.ascontiguousarray(row, dtype=np.uint32).view(np.uint8), bitorder="little")).tolist()


class _Reads:
    """The read rounds of run_reads: every kind computes what the oracles expect from the generator's own names and the oracle's live relationships, and --
    unless the run is a dry one (e is None) -- holds the engine's answer to it.  Every draw comes from `rr`, never from the write stream's generator."""

    def __init__(self, rr, names, schema_text, combine, recycle, o, e, live, stats, depth_case, cyclic, clock=None):
        from oracle.pyoracle import parse_schema
        self.rr, self.names, self.schema, self.combine, self.recycle, self.o, self.e, self.live, self.stats = rr, names, schema_text, combine, recycle, o, e, live, stats
        self.depth_case, self.cyclic, self.clock = depth_case, cyclic, clock
        self.clock_moves = 0     # moves with every clock move (an expiring run)
        self.expiry = {}         # the live relationships' expiries (an expiring run: rels() reads them from the oracle)
        self.watch = None        # kind h: the two watch sets, once opened
        self.defs = parse_schema(schema_text)
        self.nonmono = nonmono_members(self.defs)
        self.targets = [(t, m) for t, d in self.defs.items() for m in d.members]  # every relation and permission, in slot order
        self.version = 0         # moves with every accepted write
        self.compactions = 0     # the engine's snapshot_compactions / ids_recycled as of the last look
        self.recycled = 0
        self.round_no = 0
        self.cursors = []        # kind f: the cursors held open
        self.subject_targets = 0  # depth case: LookupSubjects targets asked so far
        self._rels = (-1, None)
        self._tables = None
        self._schema_names = None

    # ---- the generator's side of the names
    def rels(self):
        """the live relationships as 6-tuples (cached until the next accepted write)"""
        from oracle import orc
        key = (self.version, self.clock_moves)
        if self._rels[0] != key:
            if self.clock is None:
                self._rels = (key, [orc.parse_rel(t) for t in sorted(self.live)])
            else:  # (what the oracle reads at its clock, with the expiries the checkers carry into their replays)
                rows = sorted(x for t in ("group", "namespace", "pod") for x in self.o.read(rtype=t))
                self._rels = (key, [x[:6] for x in rows])
                self.expiry = {x[:6]: x[6] for x in rows}
        return self._rels[1]

    def now(self):
        return self.clock.now if self.clock is not None else 0

    def replay_at(self):
        """what a witness replay carries besides the hops: their expiries and the clock (an expiring run; otherwise nothing, as before)"""
        return dict(expires=self.expiry, now=self.now()) if self.clock is not None else {}

    def proof_over(self):
        """the relationships a ProofChecker is built over, with their expiries and the clock in an expiring run"""
        return (self.rels_with_expiry(), self.now()) if self.clock is not None else (self.rels(),)

    def rels_with_expiry(self):
        rels = self.rels()
        return {r: self.expiry.get(r, 0) for r in rels}

    def names_of(self, t):
        """every name of type `t` the generator knows: the universe, `stranger`, and the names in the live relationships"""
        users, groups, nss, pods = self.names
        out = set({"user": users + ["stranger"], "group": groups, "namespace": nss, "pod": pods}[t])
        for r in self.rels():
            if r[0] == t:
                out.add(r[1])
            if r[3] == t and r[4] != "*":
                out.add(r[4])
        return sorted(out)

    def resources_with_relationships(self, t):
        return sorted({r[1] for r in self.rels() if r[0] == t})

    def first_seen_in_stream(self, t):
        """names of type `t` in the live relationships that the universe does not hold: they were first named by a write of this stream"""
        users, groups, nss, pods = self.names
        known = set({"user": users, "group": groups, "namespace": nss, "pod": pods}[t])
        return [n for n in self.resources_with_relationships(t) if n not in known]

    def look_at_engine(self):
        if self.e is not None:
            st = self.e.stats()
            self.compactions, self.recycled = int(st["snapshot_compactions"]), int(st["ids_recycled"])

    def items(self, named):
        """named items as acl_item_t records: every name goes through acl_intern (a name the snapshot has never seen gets its id here)"""
        import numpy as np
        import aclgpu
        e = self.e
        if self._tables is None:
            self._tables = ({t: e.type_id(t) for t in self.defs}, {(t, m): e.relation_id(t, m) for t, d in self.defs.items() for m in d.members})
        tid, rid_ = self._tables
        out = np.zeros(len(named), dtype=aclgpu.ITEM_DTYPE)
        for i, (rt, rid, perm, st, sid, srel) in enumerate(named):
            out[i] = (tid[rt], rid_[(rt, perm)], e.intern(rt, rid), tid[st], rid_[(st, srel)] if srel else aclgpu.NO_RELATION, e.intern(st, sid))
        return out

    def schema_names(self):
        if self._schema_names is None:
            e = self.e
            self._schema_names = ({e.type_id(t): t for t in self.defs}, {(e.type_id(t), e.relation_id(t, m)): m for t, d in self.defs.items() for m in d.members})
        return self._schema_names

    def hop_names(self, raw):
        """acl_explain_hop_t records -> relationship 6-tuples (a hop is a stored relationship: both its ids are live, their names are their own)"""
        e = self.e
        tname, rname = self.schema_names()
        out = []
        for h in raw:
            rt, st = tname[int(h["rtype"])], tname[int(h["stype"])]
            sid = "*" if int(h["flags"]) & 1 else e.object_name(st, int(h["sid"]))
            srel = "" if int(h["srel"]) == 0xFFFF else rname[(int(h["stype"]), int(h["srel"]))]
            out.append((rt, e.object_name(rt, int(h["rid"])), rname[(int(h["rtype"]), int(h["relation"]))], st, sid, srel))
        return out

    def absent_names(self, raw, named_item):
        """acl_item_t records of a proof's absences -> Check items; the subject is the item's own (asserted by id), so its name is the generator's"""
        e = self.e
        tname, rname = self.schema_names()
        out = []
        for a in raw:
            rt, st = tname[int(a["resource_type"])], tname[int(a["subject_type"])]
            srel = "" if int(a["subject_relation"]) == 0xFFFF else rname[(int(a["subject_type"]), int(a["subject_relation"]))]
            sid = named_item[4] if (st == named_item[3] and int(a["subject_id"]) == e.intern(st, named_item[4])) else e.object_name(st, int(a["subject_id"]))
            out.append((rt, e.object_name(rt, int(a["resource_id"])), rname[(int(a["resource_type"]), int(a["permission"]))], st, sid, srel))
        return out

    # ---- a. LookupSubjects
    def subjects_expected(self, rt, perm, st, srel, rids, contract_cache):
        """per resource: (ids, wildcard, excluded) by name, or "DEPTH".  C4: the C oracle's Check over every name; combine: the contract of
        tests/subjects_contract.py through the Python oracle"""
        names = [n for n in self.names_of(st)]
        if st == rt:  # (a resource the call interns is a name of the subject type too -- one nobody has written holds its own `st#srel` state and nothing else)
            names = sorted(set(names) | set(rids))
        if not self.combine:
            return [({s for s in names if self.o.check(rt, rid, perm, st, s, srel) == (2, 0)}, False, set()) for rid in rids]
        from tests.subjects_contract import SubjectsContract
        if st not in contract_cache:
            contract_cache[st] = SubjectsContract(self.schema, self.rels(), st)
        return [contract_cache[st].answer(rt, rid, perm, srel, names) for rid in rids]

    def subjects_compare(self, where, rt, perm, st, srel, rids, want):
        """one acl_lookup_subjects_batch call against `want`; a resource whose contract is DEPTH fails the whole call"""
        import aclgpu
        e = self.e
        ids = [e.intern(rt, r) for r in rids]
        if any(w == "DEPTH" for w in want):
            try:
                e.lookup_subjects_ids_batch(rt, perm, st, srel, ids, want_excluded=True)
            except aclgpu.AclError as x:
                assert x.code == aclgpu.ERR_DEPTH, f"{where}: {x}"
                return None
            raise AssertionError(f"{where}: the contract of {[r for r, w in zip(rids, want) if w == 'DEPTH']} is DEPTH, the engine answered")
        bms, counts, flags, ex = e.lookup_subjects_ids_batch(rt, perm, st, srel, ids, want_excluded=True)
        for i, (rid, (wids, wild, wex)) in enumerate(zip(rids, want)):
            got = set(e.bitmap_names(st, bms[i]))
            assert got == wids, f"{where}: {rt}:{rid}#{perm} subjects {st}#{srel}: engine only {sorted(got - wids)[:5]}, contract only {sorted(wids - got)[:5]}"
            assert int(counts[i]) == len(_ids_of(bms[i])) == len(wids), f"{where}: {rt}:{rid}#{perm}: count {int(counts[i])}, row {len(_ids_of(bms[i]))}, contract {len(wids)}"
            assert bool(flags[i] & 1) == wild, f"{where}: {rt}:{rid}#{perm}: wildcard flag {int(flags[i])}, contract {wild}"
            gex = set(e.bitmap_names(st, ex[i]))
            assert gex == wex, f"{where}: {rt}:{rid}#{perm}: excluded {sorted(gex ^ wex)[:5]}"
        return bms, counts, flags

    def round_subjects(self, step):
        import numpy as np
        rr, e, st_ = self.rr, self.e, self.stats
        where = f"step {step} (LookupSubjects)"
        perms = [("pod", "view"), ("namespace", "view"), ("group", "member")]
        if self.combine:
            perms += [("pod", "audit"), ("pod", "edit"), ("pod", "hidden"), ("pod", "everywhere"), ("pod", "vetted"), ("group", "active")]
        cache = {}
        if self.depth_case:  # one target a round, three in all: picked on the oracle side, by turns a resource with a Check that ends at the depth limit and one without
            rt, perm = rr.choice([("pod", "view"), ("pod", "hidden"), ("pod", "edit")])
            users = self.names_of("user")
            pool = self.resources_with_relationships(rt)
            rr.shuffle(pool)
            want_err = self.subject_targets % 2 == 0
            if want_err:  # a user whose LookupResources fails has a candidate whose Check errs: that resource's LookupSubjects reaches the user and must fail too
                from tests.subjects_contract import SubjectsContract
                cache["user"] = SubjectsContract(self.schema, self.rels(), "user")
                u = next((u for u in rr.sample(users, 40) if self.lookup_expected(rt, perm, "user", u)[0] == "err"), None)
                pick = u and next((r for r in pool if self.o.check(rt, r, perm, "user", u)[1] and cache["user"].relaxed.check(rt, r, perm, "user", u) == "HAS"), None)
            else:
                pick = next((r for r in pool[:40] if not any(self.o.check(rt, r, perm, "user", u)[1] for u in users)), None)
            if pick is None:
                return False
            self.subject_targets += 1
            want = self.subjects_expected(rt, perm, "user", "", [pick], cache)
            st_["subj_rows"] += 1
            st_["subj_depth"] += want[0] == "DEPTH"
            st_["subj_nonempty"] += want[0] != "DEPTH" and bool(want[0][0])
            if e is not None:
                self.subjects_compare(where, rt, perm, "user", "", [pick], want)
            return True
        rt, perm = rr.choice(perms)
        # 1, 5 or 33 resources by turns; on the combine schema 33 once a run (the contract's Python oracles need 0.1 s a resource)
        n = (5, 1, 33)[self.stats["rounds_subjects"] % 3] if not self.combine or self.stats["rounds_subjects"] < 3 else (5, 1)[self.stats["rounds_subjects"] % 2]
        pool = self.resources_with_relationships(rt)
        if self.combine:  # (most pods grant `audit`, `everywhere` or `vetted` to nobody: four resources in five come from those that some of forty random users hold the permission on)
            held = set()
            for u in rr.sample(self.names[0], 40):
                if len(held) >= n:
                    break
                w = self.lookup_expected(rt, perm, "user", u)
                held |= (w[1] if w[0] == "ok" else set()) & set(pool)
            held = sorted(held)
            rr.shuffle(held)
            rest = [r for r in pool if r not in set(held)]
            rr.shuffle(rest)
            pool = [held.pop() if held and (i % 5 or not rest) else rest.pop() for i in range(min(40, len(pool)))]
        empty ={"pod": "n0/", "namespace": "", "group": ""}[rt] + f"nothing-{self.round_no}"  # interned by this call, never written
        if n == 1:  # (the batch is one resource with relationships -- under recycling a name first seen in this stream; the empty one is asked alone below)
            rids = rr.sample(self.first_seen_in_stream(rt) if self.recycle and self.first_seen_in_stream(rt) else pool, 1)
            st_["subj_first_seen"] += rids[0] in self.first_seen_in_stream(rt)
        else:
            extra = [empty]
            if self.recycle and self.first_seen_in_stream(rt):
                extra.append(rr.choice(self.first_seen_in_stream(rt)))
                st_["subj_first_seen"] += 1
            rids = list(dict.fromkeys(extra + rr.sample(pool, min(len(pool), n - len(extra)))))
        want = self.subjects_expected(rt, perm, "user", "", rids, cache)
        want_empty = self.subjects_expected(rt, perm, "user", "", [empty], cache) if n == 1 else None
        k = rr.randrange(len(rids))
        g_rid = rr.choice(rids)
        want_g = self.subjects_expected(rt, perm, "group", "member", [g_rid], cache)
        for w in want + (want_empty or []):
            st_["subj_rows"] += 1
            st_["subj_depth"] += w == "DEPTH"
            st_["subj_nonempty"] += w != "DEPTH" and bool(w[0])
            st_["subj_empty"] += w != "DEPTH" and not w[0] and not w[1]
            st_["subj_wildcard"] += w != "DEPTH" and w[1]
        st_["subj_interned_only"] += 1
        if e is None:
            return True
        got = self.subjects_compare(where, rt, perm, "user", "", rids, want)
        if want_empty is not None:
            self.subjects_compare(where, rt, perm, "user", "", [empty], want_empty)
        if got is not None:  # the n = 1 call equals its row of the batch; the string form answers the same by name
            b1, c1, f1 = e.lookup_subjects_ids_batch(rt, perm, "user", "", [e.intern(rt, rids[k])])
            words = min(b1.shape[1], got[0].shape[1])
            assert np.array_equal(b1[0][:words], got[0][k][:words]) and not b1[0][words:].any() and c1[0] == got[1][k] and f1[0] == got[2][k], f"{where}: n = 1 row of {rt}:{rids[k]}#{perm}"
            assert e.lookup_subjects(rt, rids[k], perm, "user") == want[k], f"{where}: string form of {rt}:{rids[k]}#{perm}"
        self.subjects_compare(where + " group#member", rt, perm, "group", "member", [g_rid], want_g)
        return True

    # ---- b. Explain witness
    def explain_items(self, n):
        rr = self.rr
        users, groups, nss, pods = self.names
        qs = [rand_query(rr, self.names, self.combine) for _ in range(n)]
        if self.combine:  # group#member is the one monotone permission rand_query asks on this schema: relations without `-`, `&`, `.all()` beneath fill the round up
            for _ in range(n):
                k = rr.randrange(4)
                u = rr.choice(users)
                qs.append(("group", rr.choice(groups), "member", "user", u, "") if k == 0 else ("namespace", rr.choice(nss), "viewer", "user", u, "") if k == 1 else
                          ("pod", rr.choice(pods), "auditor", "user", u, "") if k == 2 else ("group", rr.choice(groups), "member", "group", rr.choice(groups), "member"))
        return qs

    def round_explain(self, step):
        import aclgpu
        from tests import explain_checker as X
        rr, e, o, st_ = self.rr, self.e, self.o, self.stats
        qs = self.explain_items(rr.choice([64, 150, 300]) // (2 if self.combine else 1))
        want = [tuple(o.check(*q)) for q in qs]
        st_["explain_items"] += len(qs)
        granted_mono = [i for i, (q, w) in enumerate(zip(qs, want)) if w == (2, 0) and (q[0], q[2]) not in self.nonmono]
        st_["witnesses"] += len(granted_mono)
        st_["replayed"] += min(32, len(granted_mono))
        if e is None:
            return True
        perm, err, flags, off, raw = e.explain_ids(self.items(qs))
        relset = set(self.rels())
        replayed = 0
        for i, q in enumerate(qs):
            where = f"step {step} (Explain) {q} (item {i})"
            assert (int(perm[i]), int(err[i])) == want[i], f"{where}: engine {(int(perm[i]), int(err[i]))}, oracle {want[i]}"
            hops = raw[off[i]:off[i + 1]]
            if want[i] != (2, 0):
                assert int(flags[i]) == 0 and not len(hops), f"{where}: not granted, flags {int(flags[i])}, {len(hops)} hops"
            elif (q[0], q[2]) in self.nonmono:
                assert int(flags[i]) == aclgpu.EXPLAIN_UNSUPPORTED and not len(hops), f"{where}: flags {int(flags[i])}, {len(hops)} hops"
            else:
                assert int(flags[i]) == aclgpu.EXPLAIN_WITNESS, f"{where}: granted by a monotone permission, flags {int(flags[i])}"
                try:
                    X.check_witness(self.schema, relset, q, self.hop_names(hops), replay_it=replayed < 32, **self.replay_at())
                except AssertionError as x:
                    raise AssertionError(f"{where}: {x}") from None
                replayed += 1
        return True

    # ---- c. Explain proof
    def round_proof(self, step):
        import aclgpu
        from tests import proof_checker as P
        rr, e, o, st_ = self.rr, self.e, self.o, self.stats
        users, groups, nss, pods = self.names
        qs = [rand_query(rr, self.names, True) for _ in range(48)]
        for _ in range(48):
            k = rr.randrange(7)
            u = rr.choice(users)
            qs.append(("group", rr.choice(groups), "active", "user", u, "") if k == 6 else
                      ("pod", rr.choice(pods), ("audit", "edit", "hidden", "everywhere", "vetted", "view")[k], "user", u, ""))
        want = [tuple(o.check(*q)) for q in qs]
        granted = [i for i, w in enumerate(want) if w == (2, 0)]
        st_["proof_items"] += len(qs)
        st_["proofs"] += len(granted)
        if e is None:
            P.ProofChecker(self.schema, *self.proof_over())  # (the dry run pays for the checker's oracles as the real one does)
            return True
        chk = P.ProofChecker(self.schema, *self.proof_over())
        perm, err, flags, off, raw, aoff, araw = e.explain_proof_ids(self.items(qs))
        for i, q in enumerate(qs):
            where = f"step {step} (Explain proof) {q} (item {i})"
            assert (int(perm[i]), int(err[i])) == want[i], f"{where}: engine {(int(perm[i]), int(err[i]))}, oracle {want[i]}"
            hops, absent = raw[off[i]:off[i + 1]], araw[aoff[i]:aoff[i + 1]]
            if want[i] != (2, 0):
                assert int(flags[i]) == 0 and not len(hops) and not len(absent), f"{where}: not granted, flags {int(flags[i])}"
                continue
            assert int(flags[i]) == (aclgpu.EXPLAIN_PROOF if (q[0], q[2]) in self.nonmono else aclgpu.EXPLAIN_WITNESS), f"{where}: granted, flags {int(flags[i])}"
            try:
                chk.check(q, self.hop_names(hops), self.absent_names(absent, q))
            except AssertionError as x:
                raise AssertionError(f"{where}: {x}") from None
        return True

    # ---- d. Explain denial
    def round_denial(self, step):
        import aclgpu
        from tests import denial_checker as D
        rr, e, st_ = self.rr, self.e, self.stats
        orcs = D.Oracles(self.schema, self.rels_with_expiry(), self.now())
        cand = [q for q in self.explain_items(120) if (q[0], q[2]) not in self.nonmono]
        denied = []
        for q in dict.fromkeys(cand):
            if orcs.denied(q):
                denied.append(q)
                if len(denied) == 8:
                    break
        if not denied:
            return False
        # the restatement's own answer: which of them have a grant at all, and -- in a dry run -- the lists the checker is timed on
        restated = [D.grants_of(orcs.defs, D.closure(orcs.defs, orcs.rels, q[:3], self.now()), q[3], q[5]) for q in denied]
        st_["denied_items"] += len(denied)
        st_["denied_with_grants"] += sum(bool(g) for g in restated)
        if e is None:
            for k, (q, g) in enumerate(zip(denied, restated)):
                D.check_grants(orcs, q, [(t, o_, m, lv) for (t, o_, m), lv in g.items()], seed=step)
            return True
        perm, err, flags, off, recs = e.explain_denial_ids(self.items(denied))
        for k, q in enumerate(denied):
            where = f"step {step} (Explain denial) {q}"
            assert (int(perm[k]), int(err[k])) == (1, 0), f"{where}: engine {(int(perm[k]), int(err[k]))}, the oracles deny it without error"
            assert int(flags[k]) == aclgpu.EXPLAIN_DENIAL, f"{where}: flags {int(flags[k])}"
            grants = D.name_grants(e, self.schema, recs[off[k]:off[k + 1]])
            assert bool(grants) == bool(restated[k]), f"{where}: {len(grants)} grants, the closure has {len(restated[k])}"
            try:  # (every grant written alone grants the item at its level, by both oracles; no other single write does)
                D.check_grants(orcs, q, grants, seed=step)
            except AssertionError as x:
                raise AssertionError(f"{where}: {x}") from None
        return True

    # ---- g. Explain for revocation
    def round_revoke(self, step):
        """granted monotone items of the stream: the engine's cut set of each -- the single deletes that revoke it -- is the brute force's (one relationship out,
        every item asked, the relationship back, for EVERY live relationship, by the C oracle), and goes through tests/revoke_checker.py (every cut revokes by both
        oracles, with the expiries and the clock of the store)"""
        import aclgpu
        from tests import revoke_checker as R
        rr, e, o, st_ = self.rr, self.e, self.o, self.stats
        cand = [q for q in dict.fromkeys(self.explain_items(150)) if (q[0], q[2]) not in self.nonmono and tuple(o.check(*q)) == (2, 0)]
        items = cand[:12]
        if not items:
            return False
        from tests import denial_checker as D
        ck = R.Checker(self.schema, self.rels_with_expiry(), self.now())
        # (the brute force over every relationship of the OBJECTS some item's Check looks at -- tests/denial_checker.py closure(), the items are monotone: a
        # relationship of an object no Check reaches cannot change an answer; on the cyclic graphs the C oracle needs a millisecond per denied Check)
        objects = set()
        for q in items:
            objects |= {s[:2] for s in D.closure(ck.orcs.defs, ck.orcs.rels, q[:3], self.now())}
        want = ck.brute(items, only=[r for r in ck.orcs.rels if r[:2] in objects])
        ck._cuts.update(want)
        assert list(want) == items, f"step {step} (Explain revoke): the checker's oracles grant {len(want)} of {len(items)} items the stream's oracle grants"
        st_["revoke_items"] += len(items)
        st_["revoke_with_cuts"] += sum(bool(c) for c in want.values())
        st_["revoke_cuts"] += sum(len(c) for c in want.values())
        if e is None:
            return True
        perm, err, flags, off, raw = e.explain_revoke_ids(self.items(items))
        for i, q in enumerate(items):
            where = f"step {step} (Explain revoke) {q} (item {i})"
            assert (int(perm[i]), int(err[i]), int(flags[i])) == (2, 0, aclgpu.EXPLAIN_REVOKE), f"{where}: engine {(int(perm[i]), int(err[i]), int(flags[i]))}, the oracles grant it"
            cuts = self.hop_names(raw[off[i]:off[i + 1]])
            assert len(set(cuts)) == len(cuts) and set(cuts) == want[q], f"{where}: engine only {sorted(set(cuts) - want[q])[:3]}, brute force only {sorted(want[q] - set(cuts))[:3]}"
            try:
                ck.check(q, cuts)
            except AssertionError as x:
                raise AssertionError(f"{where}: {x}") from None
        return True

    # ---- h. watch sets (expiring runs)
    NOBODY = "nobody-names-this-subject"

    def watch_rows(self):
        """the oracle's rows of both sets now: {user: pods} by LookupResources (None: a lookup fails), {pod: users, `*` among them} by Check per subject"""
        w = self.watch
        res = {}
        for u in w["users"]:
            out = self.lookup_expected("pod", "view", "user", u)
            if out[0] == "err":
                return None, None
            res[u] = out[1]
        users = self.names_of("user")
        sub = {}
        for p in w["pods"]:
            row = {u for u in users if tuple(self.o.check("pod", p, "view", "user", u)) == (2, 0)}
            if tuple(self.o.check("pod", p, "view", "user", self.NOBODY)) == (2, 0):
                row.add("*")
            sub[p] = row
        return res, sub

    def round_watch(self, step):
        """One resource-direction set (4 users) and one subject-direction set (4 pods) on pod#view, opened at the first round and polled at every later one: the
        records are the difference of the oracle's rows since the last poll (tests/watch_records.py) -- behind writes, and behind clock moves with no write."""
        import aclgpu
        from tests.watch_records import expected_records, records_of
        rr, e, st_ = self.rr, self.e, self.stats
        if self.watch is None:
            users, pods = rr.sample(self.names[0], 4), rr.sample(self.resources_with_relationships("pod"), 4)
            self.watch = w = dict(users=users, pods=pods, res=None, sub=None)
            if e is not None:
                w["res"], w["sub"] = e.watch_set("pod", "view", "user"), e.subject_watch_set("pod", "view", "user")
                w["wres"], w["wsub"] = [w["res"].add(u) for u in users], [w["sub"].add(p) for p in pods]  # (the watchers' ids, in the order of the names)
            w["held_res"], w["held_sub"] = {k: set() for k in w.get("wres", range(4))}, {k: set() for k in w.get("wsub", range(4))}  # (the empty rows of the adds)
        w = self.watch
        res, sub = self.watch_rows()
        if res is None:
            return False
        wres, wsub = w.get("wres", range(4)), w.get("wsub", range(4))
        after_res, after_sub = {wres[k]: res[u] for k, u in enumerate(w["users"])}, {wsub[k]: sub[p] for k, p in enumerate(w["pods"])}
        behind_clock = self.clock is not None and self.clock.moved_last
        for d, held, after in (("res", w["held_res"], after_res), ("sub", w["held_sub"], after_sub)):
            lost = sum(len(held[k] - after[k]) for k in after)
            st_["watch_changes_" + d] += lost + sum(len(after[k] - held[k]) for k in after)
            st_["watch_loss_behind_clock_" + d] += bool(lost) and behind_clock
        st_["watch_polls"] += 1
        if e is not None:
            where = f"step {step} (watch sets{', behind a clock move' if behind_clock else ''})"
            wid = e.find("user", "*")
            want = expected_records(w["held_res"], after_res, lambda n: e.intern("pod", n))
            got = records_of(w["res"].poll()[1])
            assert got == want, f"{where}: resource direction: engine only {sorted(set(got) - set(want))[:4]}, oracle only {sorted(set(want) - set(got))[:4]}"
            want = expected_records(w["held_sub"], after_sub, lambda n: wid if n == "*" else e.intern("user", n), lambda i: aclgpu.WATCH_CHANGE_WILDCARD if i == wid else 0)
            got = records_of(w["sub"].poll()[1], reserved=True)
            assert got == want, f"{where}: subject direction: engine only {sorted(set(got) - set(want))[:4]}, oracle only {sorted(set(want) - set(got))[:4]}"
        w["held_res"], w["held_sub"] = after_res, after_sub
        return True

    # ---- e. multi-target LookupResources
    def lookup_expected(self, rt, pm, st, sid, srel=""):
        """("ok", names) or ("err", code): a lookup whose candidate's Check errs fails as a whole"""
        try:
            return ("ok", set(self.o.lookup(rt, pm, st, sid, srel)))
        except Exception as ex:  # noqa: BLE001
            if getattr(ex, "code", None) is None:
                raise
            return ("err", ex.code)

    def round_multi(self, step):
        import numpy as np
        import aclgpu
        rr, e, st_ = self.rr, self.e, self.stats
        users = self.names_of("user")
        # 1, 3 or 20 subjects by turns; with group cycles 20 once a run (the oracle's brute-force lookups need 20 ms a row there), and never in the depth case
        k = self.stats["rounds_multi"]
        subs = rr.sample(users, (1, 1, 1, 1, 1, 3)[k % 6] if self.depth_case else (3, 1)[k % 2] if self.cyclic and k >= 3 else (3, 1, 20)[k % 3])
        targets = self.targets
        want = [[self.lookup_expected(rt, pm, "user", u) for u in subs] for rt, pm in targets]
        failing = [j for j in range(len(targets)) if any(w[0] == "err" for w in want[j])]
        st_["multi_rows"] += len(subs) * len(targets)
        st_["multi_failing_targets"] += len(failing)
        review_u = rr.randrange(len(subs))
        if e is None:
            return True
        where = f"step {step} (multi-target lookup, {len(subs)} subjects)"
        sids = [e.intern("user", u) for u in subs]
        singles = {}
        for j, (rt, pm) in enumerate(targets):  # every target alone: its rows by name against the oracle, or its failure
            if j in failing:
                try:
                    e.lookup_ids_batch(rt, pm, "user", "", sids)
                except aclgpu.AclError as x:
                    assert x.code == aclgpu.ERR_DEPTH, f"{where}: {rt}#{pm}: {x}"
                    continue
                raise AssertionError(f"{where}: the oracle fails {rt}#{pm}, the engine answered")
            singles[j] = e.lookup_ids_batch(rt, pm, "user", "", sids)
            for i, u in enumerate(subs):
                got = set(e.bitmap_names(rt, singles[j][0][i]))
                assert got == want[j][i][1], f"{where}: {rt}#{pm}@user:{u}: engine only {sorted(got - want[j][i][1])[:5]}, oracle only {sorted(want[j][i][1] - got)[:5]}"
        if failing:  # a candidate's error fails the call (no ACL_FLAG_LENIENT_LOOKUP here); the targets that answer alone still answer together
            try:
                e.lookup_ids_multi(targets, "user", "", sids)
            except aclgpu.AclError as x:
                assert x.code == aclgpu.ERR_DEPTH and "max depth exceeded" in str(x), f"{where}: {x}"
            else:
                raise AssertionError(f"{where}: the oracle fails {[targets[j] for j in failing]}, the multi call answered")
        ok = [j for j in range(len(targets)) if j not in failing]
        rows, counts = e.lookup_ids_multi([targets[j] for j in ok], "user", "", sids)
        for k, j in enumerate(ok):  # bit for bit what the single-target call answers
            assert np.array_equal(rows[k], singles[j][0]) and np.array_equal(counts[:, k], singles[j][1]), f"{where}: {targets[j]} differs from lookup_ids_batch"
        u = subs[review_u]
        try:
            rev = e.access_review("user", u)
        except aclgpu.AclError as x:
            assert x.code == aclgpu.ERR_DEPTH and any(want[j][review_u][0] == "err" for j in range(len(targets))), f"{where}: access_review of {u}: {x}"
        else:
            assert all(want[j][review_u][0] == "ok" for j in range(len(targets))), f"{where}: access_review of {u} answered, the oracle fails a target"
            assert rev == {t: want[j][review_u][1] for j, t in enumerate(targets)}, f"{where}: access_review of {u}"
        return True

    # ---- f. cursors held across writes
    def cursor_chain(self, cur, row, limit):
        out, after = [], None
        while True:
            ids, more = cur.page(row, after, limit)
            out += ids.tolist()
            if not more:
                return out
            assert len(ids), "a page says `more` and holds no id"
            after = out[-1]

    def cursor_open(self, step, kind, rt, perm, st):
        """one cursor: its expected rows by name on the oracle side; on the engine its rows paged whole, held to them by name, the ids remembered"""
        import aclgpu
        rr, e = self.rr, self.e
        where = f"step {step} (cursor open {kind} {rt}#{perm})"
        users, groups = self.names_of("user"), self.names_of("group")
        if kind == "subjects":
            keys = rr.sample(self.resources_with_relationships(rt), 3)
            want = self.subjects_expected(rt, perm, "user", "", keys, {})
            if any(w == "DEPTH" for w in want):
                want = None
            else:
                flags, want = [w[1] for w in want], [w[0] for w in want]
        else:
            keys = [("user", "", u) for u in rr.sample(users, 3)] + ([("group", "member", g) for g in rr.sample(groups, 2)] if kind == "mixed" else [])
            w = [self.lookup_expected(rt, perm, s, n, r) for s, r, n in keys]
            want, flags = (None if any(x[0] == "err" for x in w) else [x[1] for x in w]), [False] * len(keys)
        held = dict(kind=kind, row_type=st if kind == "subjects" else rt, want=want, version=self.version, clock=self.clock_moves, reads=0, cur=None, ids=None, names=None,
                    flags=flags)
        if e is None:
            return held if want is not None else None
        try:
            if kind == "subjects":
                cur = e.subjects_cursor(rt, perm, "user", "", [e.intern(rt, k) for k in keys])
            elif kind == "lookup":
                cur = e.lookup_cursor(rt, perm, "user", "", [e.intern("user", n) for _s, _r, n in keys])
            else:
                cur = e.lookup_cursor_mixed(rt, perm, [(s, r, e.intern(s, n)) for s, r, n in keys])
        except aclgpu.AclError as x:
            assert want is None and x.code == aclgpu.ERR_DEPTH, f"{where}: {x}"
            return None
        assert want is not None, f"{where}: the oracle fails a row, the engine opened the cursor"
        self.look_at_engine()
        held.update(cur=cur, ids=[], names=[], compactions=self.compactions, recycled=self.recycled)
        _rev, counts, cflags = cur.info()
        for i in range(len(keys)):
            ids = self.cursor_chain(cur, i, 500)
            pid, names, more = cur.page_names(i, None, len(ids) + 1)
            assert pid.tolist() == ids and not more and int(counts[i]) == len(ids), f"{where}: row {i}: pages, names and count disagree"
            assert set(names) == want[i] and len(names) == len(want[i]), f"{where}: row {i} ({keys[i]}): engine only {sorted(set(names) - want[i])[:5]}, oracle only {sorted(want[i] - set(names))[:5]}"
            assert bool(cflags[i] & 1) == bool(flags[i]), f"{where}: row {i}: wildcard flag {int(cflags[i])}"
            held["ids"].append(ids)
            held["names"].append(names)
        return held

    def cursor_read(self, step, h):
        """a cursor opened before at least one accepted write or clock move: its rows are what they were"""
        import aclgpu
        st_ = self.stats
        st_["cursors_read_later"] += 1
        st_["cursors_read_after_clock_move"] += self.clock_moves > h["clock"]
        h["reads"] += 1
        if self.e is None:
            return
        self.look_at_engine()
        st_["cursors_read_after_compaction"] += self.compactions > h["compactions"]
        moved = self.recycled > h["recycled"]
        st_["cursors_read_after_recycling"] += moved
        cur = h["cur"]
        for i, ids in enumerate(h["ids"]):
            where = f"step {step} (cursor {h['kind']} opened {self.version - h['version']} writes ago, row {i})"
            for limit in (1, 7, 500):
                got = self.cursor_chain(cur, i, limit)
                assert got == ids, f"{where}: limit {limit}: {len(got)} ids, {len(ids)} at the open; differ at {sorted(set(got) ^ set(ids))[:5]}"
            try:
                pid, names, _more = cur.page_names(i, None, len(ids) + 1)
            except aclgpu.AclError as x:
                assert moved and x.code == aclgpu.ERR_FAILED_PRECONDITION, f"{where}: page_names: {x}"
                st_["page_names_refused"] += 1
            else:
                assert pid.tolist() == ids and names == h["names"][i], f"{where}: page_names answers other names than at the open"

    def cursor_derive(self, step, a, b):
        """any & all & ~none over two cursors of one direction and revision: the set algebra of the remembered ids"""
        rr, e = self.rr, self.e
        rows = [(c, r) for c, h in enumerate((a, b)) for r in range(len(h["want"])) if not h["flags"][r]]  # (a wildcard row is no bitmap: derive refuses it)
        if len(rows) < 4:
            return
        self.stats["derives"] += 1
        exprs = [(rr.sample(rows, 2), rr.sample(rows, 1), rr.sample(rows, 1)) for _ in range(3)]  # (drawn in a dry run too: one stream for both)
        if e is None:
            return
        S = lambda ref: set((a, b)[ref[0]]["ids"][ref[1]])  # noqa: E731
        want = [sorted(((S(any_[0]) | S(any_[1])) & S(all_[0])) - S(none[0])) for any_, all_, none in exprs]
        counts = e.count_rows([a["cur"], b["cur"]], exprs)
        with e.derive_cursor([a["cur"], b["cur"]], exprs) as d:
            for k, w in enumerate(want):
                got = self.cursor_chain(d, k, 7)
                assert got == w and int(counts[k]) == len(w), f"step {step} (derived cursor, expression {k}): {len(got)} ids, count {int(counts[k])}, set algebra {len(w)}"

    def round_cursors(self, step):
        rr, st_ = self.rr, self.stats
        old = [h for h in self.cursors if h["version"] < self.version or h["clock"] < self.clock_moves]
        if old:
            for h in old:
                self.cursor_read(step, h)
            pairs = [(a, b) for a in old for b in old if a is not b and a.get("pair") is b]
            if pairs:
                self.cursor_derive(step, *pairs[0])
            for h in old:  # some are closed here, the rest when the engine closes
                if h["reads"] >= 3 and (h["reads"] >= 6 or rr.random() < 0.3):
                    if h["cur"] is not None:
                        h["cur"].close()
                    self.cursors[:] = [c for c in self.cursors if c is not h]  # (by identity: a pair's dicts refer to each other)
                    st_["cursors_closed"] += 1
            return True
        if len(self.cursors) >= 3:
            return False
        perms = [("pod", "view"), ("namespace", "view"), ("group", "member")] + ([("pod", "edit"), ("pod", "hidden"), ("pod", "vetted")] if self.combine else [])
        rt, perm = rr.choice(perms)
        if len(self.cursors) <= 1:  # a pair of one direction, opened on one snapshot: the sources of a derived cursor
            kinds = rr.choice([("lookup", "mixed"), ("subjects", "subjects")])
        else:
            kinds = (rr.choice(["lookup", "mixed", "subjects"]),)
        opened = [h for h in (self.cursor_open(step, k, rt, perm, "user") for k in kinds) if h is not None]
        if len(opened) == 2:
            opened[0]["pair"], opened[1]["pair"] = opened[1], opened[0]
        self.cursors += opened
        st_["cursors_opened"] += len(opened)
        return bool(opened)


def run_reads(seed: int, steps: int, schema: str = "c4", acyclic: bool = False, recycle: bool = False, compact_early: bool = False, universe: int = 1, engine: bool = True,
              verbose: bool = True, depth_case: bool = False, read_share: float = 0.75, expiring: bool = False, probe: int = 200) -> dict:
    """The read paths the Check campaign does not reach, on the same kind of live graph: between run()'s writes (TOUCH / CREATE / DELETE batches, filter
    deletes) a step is, with probability `read_share`, one read round -- LookupSubjects, Explain witness, Explain proof (combine schema), Explain denial,
    Explain for revocation, multi-target LookupResources with access_review, or cursors held open across the writes (paged, named, derived, counted) -- each
    held to the oracles.  expiring: the schema's expiring variant under a Clock -- one step in four moves the clock instead of writing (the probe batch around it),
    every round kind runs against the oracle at the current clock, the checkers replay with the hops' expiries, cursors are read across clock moves, and a
    `watch` round polls a resource-direction and a subject-direction watch set against the difference of the oracle's rows.
    engine=False: the oracle's half alone, same stream, same expected values, no GPU: what a case costs on the oracle side and whether its stream covers what
    it is for.  depth_case: kinds a and e only, one LookupSubjects target a round and three in all (a cyclic combine graph: the Python oracle needs over a second
    per target there), picked by turns with and without a Check that ends at the depth limit.  -> stats."""
    from oracle import orc
    combine = schema == "combine"
    schema_text = schema_text_of(schema, expiring)
    rng = random.Random(seed)
    rr = random.Random(f"reads/{seed}")  # (the write stream's generator is never drawn from by a read)
    names = make_universe(rng, universe)
    rand_tuple = make_rand_tuple(rng, names, combine, recycle, acyclic)
    e = open_engine(schema_text, recycle, compact_early) if engine else None
    o = orc.Oracle(schema_text)
    live = set()
    stats = {k: 0 for k in ("writes", "write_errors", "filter_deletes", "writes_accepted", "rounds", "skipped", "subj_rows", "subj_nonempty", "subj_empty", "subj_depth",
                            "subj_wildcard", "subj_interned_only", "subj_first_seen", "explain_items", "witnesses", "replayed", "proof_items", "proofs", "denied_items",
                            "denied_with_grants", "multi_rows", "multi_failing_targets", "cursors_opened", "cursors_read_later", "cursors_read_after_compaction",
                            "cursors_read_after_recycling", "page_names_refused", "cursors_closed", "derives", "cursors_read_after_clock_move", "revoke_items",
                            "revoke_with_cuts", "revoke_cuts", "watch_polls", "watch_changes_res", "watch_changes_sub", "watch_loss_behind_clock_res",
                            "watch_loss_behind_clock_sub")}
    clock = Clock(rng, seed, names, combine, o, [e], stats, probe) if expiring else None
    load_initial(rand_tuple, o, e, live, universe, clock)
    reads = _Reads(rr, names, schema_text, combine, recycle, o, e, live, stats, depth_case, not acyclic, clock)
    kinds = ["subjects", "multi"] if depth_case else ["subjects", "explain", "explain", "denial", "multi", "cursors", "cursors", "revoke"] + (["proof"] if combine else []) + \
        (["watch"] if expiring else [])

    def probe_check(qs, want, where):
        perms, errs = e.check_bulk(qs)
        for i, q in enumerate(qs):
            assert (perms[i], errs[i]) == want[i], f"{where}: probe check {q} (item {i}): engine {(perms[i], errs[i])}, oracle {want[i]}"
    for k in dict.fromkeys(kinds):
        stats["rounds_" + k], stats["seconds_" + k] = 0, 0.0
    todo = []
    t0 = time.time()
    for step in range(steps):
        if clock is not None and rng.random() < 0.25:  # (no write: the read round behind it sees the relationships whose liveness changed)
            clock.move(step, live, probe_check if e is not None else None)
            reads.clock_moves += 1
            accepted = False
        elif rng.random() < 0.9:
            accepted = write_batch(rng, step, rand_tuple, o, e, live, 25, stats, clock)
        else:
            accepted = filter_delete(rng, step, names, combine, o, e, live, stats, clock) > 0
        if accepted:
            reads.version += 1
            stats["writes_accepted"] += 1
        if rr.random() < read_share:
            if not todo:  # every enabled kind once (cursors twice) in a shuffled order, then again
                # (the kinds whose oracle side is dear -- LookupSubjects, denial, multi-target lookups outside the depth case -- run four rounds, then the cheap ones go on)
                todo = [k for k in kinds if not (k == "subjects" and depth_case and reads.subject_targets >= 3) and
                        not (k in ("subjects", "denial", "multi", "revoke") and not depth_case and stats["rounds_" + k] >= 4) and
                        not (k == "watch" and stats["rounds_watch"] >= 9)]  # (the first watch round opens the sets, eight polls follow)
                rr.shuffle(todo)
            kind = todo.pop()
            reads.round_no += 1
            t1 = time.time()
            done = getattr(reads, "round_" + kind)(step)
            stats["seconds_" + kind] = round(stats["seconds_" + kind] + time.time() - t1, 2)
            stats["rounds"] += 1
            stats["rounds_" + kind] += bool(done)
            stats["skipped"] += not done
        if verbose and step % 10 == 9:
            print(f"step {step + 1}/{steps}: {stats}, {len(live)} relationships, {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
    if not depth_case and not reads.cursors:  # (at least one cursor is still open when the engine closes)
        reads.cursors += [h for h in [reads.cursor_open(steps, "lookup", "group", "member", "user")] if h is not None]
    stats["cursors_left_open"] = len(reads.cursors)
    stats["seconds"] = round(time.time() - t0, 1)
    if e is not None:
        if reads.watch is not None:
            reads.watch["res"].close()
            reads.watch["sub"].close()
        st = e.stats()
        stats.update({k: int(st[k]) for k in ("snapshot_builds", "snapshot_patches", "snapshot_compactions", "ids_recycled", "rev_multi_passes") if k in st})
        e.close()  # (with the cursors still held: the engine closes them)
    return stats


def run_patcher(seed: int, steps: int, universe: int = 1, burst: int = 25, shard=None, schema: str = "c4", expiring: bool = False) -> dict:
    """No GPU: the same kind of write stream on a STORE-ONLY engine, and after every write the host snapshot is brought up to date the way a read
    would (patched in place, or rebuilt) and verified against the store (acl_selfcheck_snapshot: every relationship findable by the kernels'
    search, nothing dead left, rows sorted, no unsound leaf flag).  -> how often it was patched (1), rebuilt (0) or current (2).
    expiring: the schema's expiring variant under a Clock -- two TOUCHes in five carry an expiry, one step in four moves the clock instead of writing, and after
    every step ReadRelationships of the store equals the C oracle's; "rebuilt_outside_adoption": rebuilds at a step that adopted no background build,
    "dropped_after_expiry" / "adopted_after_expiry": background builds dropped / adopted with an expiry passed (by the oracle's read difference) between their
    two halves -- the hook's second half replays the crossings onto the build with the patcher and verifies the adopted snapshot against the store."""
    import aclgpu
    from oracle import orc

    rng = random.Random(seed)
    users = [f"u{i}" for i in range(160 * universe)]
    groups = [f"g{i}" for i in range(48 * universe)]
    nss = [f"n{i}" for i in range(8 * universe)]
    pods = [f"{rng.choice(nss)}/p{i}" for i in range(240 * universe)]
    shapes = [lambda: f"group:{rng.choice(groups)}#member@group:{rng.choice(groups)}#member", lambda: f"group:{rng.choice(groups)}#member@user:{rng.choice(users)}",
              lambda: f"pod:{rng.choice(pods)}#namespace@namespace:{rng.choice(nss)}", lambda: f"pod:{rng.choice(pods)}#creator@user:{rng.choice(users)}",
              lambda: f"namespace:{rng.choice(nss)}#creator@user:{rng.choice(users)}", lambda: f"pod:{rng.choice(pods)}#viewer@user:{rng.choice(users)}",
              lambda: f"pod:{rng.choice(pods)}#viewer@group:{rng.choice(groups)}#member", lambda: f"namespace:{rng.choice(nss)}#viewer@user:{rng.choice(users)}",
              lambda: f"namespace:{rng.choice(nss)}#viewer@group:{rng.choice(groups)}#member"]
    if schema == "combine":  # wildcard classes, a non-monotone userset subject, the relations behind `-` and `&`
        shapes += [lambda: f"group:{rng.choice(groups)}#banned@user:{rng.choice(users)}", lambda: f"namespace:{rng.choice(nss)}#banned@group:{rng.choice(groups)}#member",
                   lambda: f"namespace:{rng.choice(nss)}#viewer@user:*", lambda: f"pod:{rng.choice(pods)}#viewer@group:{rng.choice(groups)}#active",
                   lambda: f"pod:{rng.choice(pods)}#auditor@group:{rng.choice(groups)}#member", lambda: f"pod:{rng.choice(pods)}#banned@user:*",
                   lambda: f"pod:{rng.choice(pods)}#banned@user:{rng.choice(users)}", lambda: f"pod:{rng.choice(pods)}#auditor@user:{rng.choice(users)}"]
    e = aclgpu.Engine(schema_text_of(schema, expiring), store_only=True)
    codes = {0: 0, 1: 0, 2: 0, "adopted": 0, "dropped": 0}
    o = clock = None
    if expiring:
        o = orc.Oracle(schema_text_of(schema, True))
        codes.update(rebuilt_outside_adoption=0, dropped_after_expiry=0, adopted_after_expiry=0)
        clock = Clock(rng, seed, (users, groups, nss, pods), schema == "combine", o, [e], codes, probe=40)

    def expires(t):  # -> () or (expiry,)
        at = clock.expiry_for(t, refusable=False) if clock is not None else 0
        return (at,) if at else ()

    def same_read(where):
        a, b = sorted(x for t in ("group", "namespace", "pod") for x in e.read(rtype=t)), sorted(x for t in ("group", "namespace", "pod") for x in o.read(rtype=t))
        assert a == b, f"{where}: ReadRelationships differs: {sorted(set(a) ^ set(b))[:6]}"

    if shard:  # (rank, world): the snapshot of ONE shard of the type-hash layout -- it holds, and patches, only the rows of the types it owns
        e._check(e._L.acl_shard_configure(e._h, shard[0], shard[1]))
    live = set(dict.fromkeys(rng.choice(shapes)() for _ in range(2500 * universe)))
    init = sorted(live)
    for i in range(0, len(init), 500):
        ups = [(aclgpu.OP_TOUCH, t) + expires(t) for t in init[i:i + 500]]
        e.write(ups)
        if o is not None:
            o.write(ups)  # (the two sides' op codes are the same numbers)
    assert (aclgpu.OP_TOUCH, aclgpu.OP_DELETE) == (orc.OP_TOUCH, orc.OP_DELETE)
    e.selfcheck_snapshot_code()
    pending_build = None
    expired_since_build = False
    for step in range(steps):
        adopted_here = False
        if clock is not None and rng.random() < 0.25:
            gone = clock.move(step, live)[1]
            expired_since_build = expired_since_build or bool(gone)
        elif rng.random() < 0.9:
            pool = sorted(live)
            ups = {}
            for _u in range(rng.randrange(1, burst)):
                t = rng.choice(shapes)() if rng.random() < 0.55 or not pool else rng.choice(pool)
                op = aclgpu.OP_TOUCH if t not in live or rng.random() < 0.3 else aclgpu.OP_DELETE
                ups[t] = (op, t) + (expires(t) if op == aclgpu.OP_TOUCH else ())
            e.write(list(ups.values()))
            if o is not None:
                o.write(list(ups.values()))
                clock.accepted(list(ups.values()), aclgpu.OP_DELETE)
            for op, t, *_ in ups.values():
                (live.discard if op == aclgpu.OP_DELETE else live.add)(t)
        else:
            f = rng.choice([dict(rtype="pod", rid=rng.choice(pods)), dict(rtype="group", rel="member", stype="user", sid=rng.choice(users))])
            n = e.delete_by_filter(**f)
            if o is not None:
                assert o.delete_by_filter(**f) == n, f"step {step}: delete_by_filter {f}"
                clock.filtered(f)
            live = set(f"{a}:{b}#{c}@{d}:{x}" + (f"#{y}" if y else "") for t in ("group", "namespace", "pod") for a, b, c, d, x, y, *_ in e.read(rtype=t))
        code = e.selfcheck_snapshot_code()  # (raises when the snapshot does not describe the store)
        codes[code] += 1
        if o is not None:
            same_read(f"step {step} (now {clock.now})")
        # a background compaction's two halves around the writes in between: build from a copy-on-write view now, adopt it some writes later
        if pending_build is None and rng.random() < (0.06 if expiring else 0.02):
            e.selfcheck_compaction(0)
            pending_build = rng.randrange(0, 8 if expiring else 30)
            expired_since_build = False
        elif pending_build is not None:
            if pending_build == 0:
                adopted_here = bool(e.selfcheck_compaction(1))  # (phase 1 verifies the adopted snapshot against the store)
                codes["adopted" if adopted_here else "dropped"] += 1
                if expiring:
                    codes["dropped_after_expiry"] += not adopted_here and expired_since_build
                    codes["adopted_after_expiry"] += adopted_here and expired_since_build
                pending_build = None
            else:
                pending_build -= 1
        if expiring:
            codes["rebuilt_outside_adoption"] += code == 0
    e.close()
    return codes


# ---------------------------------------------------------------------------------------------------------------- the sharded campaign
class _TapOracle:
    """The oracle as write_batch / filter_delete / load_initial see it: every call goes through, the last write's outcome is remembered for _TapEngine."""

    def __init__(self, o):
        self._o, self.code, self.removed = o, None, 0

    def __getattr__(self, k):
        return getattr(self._o, k)

    def write(self, ups):
        from oracle import orc
        self.code = None
        try:
            return self._o.write(ups)
        except orc.OracleError as x:
            self.code = x.code
            raise

    def delete_by_filter(self, **f):
        self.removed = self._o.delete_by_filter(**f)
        return self.removed


class _TapEngine:
    """Stands where write_batch / filter_delete / load_initial expect the engine: it writes the script -- what they send, with the outcome the oracle
    just gave -- and answers as the oracle did."""

    def __init__(self, tap, sink):
        self.tap, self.sink, self.step = tap, sink, -1

    def write(self, ups):
        import aclgpu
        self.sink.append(("write", self.step, list(ups), self.tap.code))
        if self.tap.code is not None:
            raise aclgpu.AclError(self.tap.code, "as the oracle")

    def delete_by_filter(self, **f):
        self.sink.append(("filter", self.step, dict(f), self.tap.removed))
        return self.tap.removed


class _ScriptReads(_Reads):
    """_Reads without an engine: round_subjects picks the resources as the read campaign does, and every LookupSubjects request it computes the expected rows
    of is kept for the script"""

    def __init__(self, *a):
        super().__init__(*a)
        self.asked = []

    def subjects_expected(self, rt, perm, st, srel, rids, contract_cache):
        want = super().subjects_expected(rt, perm, st, srel, rids, contract_cache)
        self.asked.append((rt, perm, st, srel, list(rids), want))
        return want


SHARD_CHECK_SIZES = (1, 7, 64, 900, 3000)


def sharded_script(seed: int, steps: int, schema: str = "c4", acyclic: bool = False, recycle: bool = False, universe: int = 1, depth_case: bool = False,
                   read_share: float = 0.75, verbose: bool = False, expiring: bool = False, probe: int = 200) -> dict:
    """Phase 1 of run_sharded (no GPU, no engine): one pass over run_reads' kind of stream with the oracles alone -> the ordered script every rank replays.
    script["init"]: the starting graph's write steps; script["steps"]: in order
      ("write", step, updates, the oracle's outcome code or None) | ("filter", step, filter, removed)
      ("clock", step, now) -- an expiring script (script["now0"]: the clock every rank starts at): every rank sets its own engine's clock before the next read
      ("check", step, [item], [(permissionship, error)]) -- with a fifth field "probe": the Clock's probe batch, answered right behind a clock step
      ("lookup", step, rtype, permission, [user], [("ok", names) | ("err", code)], [follow-up]) -- a follow-up is ("check", items, want) or ("lookup", [user], [outcome]):
          asked behind a call that must fail, the next call on that engine has to answer
      ("subjects", step, [(rtype, permission, stype, srel, [resource], [(ids, wildcard, excluded) | "DEPTH"])])
    and script["stats"], what the stream covers.  Every draw of a read comes from a generator of its own: the write stream is run_reads' for the same seed."""
    from oracle import orc
    combine = schema == "combine"
    schema_text = schema_text_of(schema, expiring)
    rng = random.Random(seed)
    rr = random.Random(f"sharded/{seed}")
    names = make_universe(rng, universe)
    users, groups, nss, pods = names
    rand_tuple = make_rand_tuple(rng, names, combine, recycle, acyclic)
    o = _TapOracle(orc.Oracle(schema_text))
    init, script = [], []
    rec = _TapEngine(o, init)
    live = set()
    stats = {k: 0 for k in ("writes", "write_errors", "filter_deletes", "writes_accepted", "writes_read_before_next", "rounds", "skipped", "rounds_check", "rounds_lookup",
                            "rounds_subjects", "check_items", "check_depth_items", "check_has_items", "check_first_seen_items", "check_outruns_expected", "lookup_rows", "lookup_calls",
                            "lookup_calls_failed", "lookup_rows_nonempty", "subj_rows", "subj_nonempty", "subj_empty", "subj_depth", "subj_wildcard", "subj_interned_only",
                            "subj_first_seen", "subj_no_relationships", "subj_calls", "subj_calls_failed", "subj_calls_answered", "subj_answered_over_arrow", "subj_wildcard_excluded",
                            "reads_behind_clock_check", "reads_behind_clock_lookup", "reads_behind_clock_subjects")}
    clock = Clock(rng, seed, names, combine, o, [], stats, probe) if expiring else None
    load_initial(rand_tuple, o, rec, live, universe, clock)
    rec.sink = script
    reads = _ScriptReads(rr, names, schema_text, combine, recycle, o, None, live, stats, depth_case, not acyclic, clock)
    lookup_perms = [("pod", "view"), ("namespace", "view"), ("group", "member")] + \
        ([("pod", "audit"), ("pod", "edit"), ("pod", "hidden"), ("group", "active"), ("pod", "everywhere"), ("pod", "vetted")] if combine else [])
    subject_rounds = 3 if depth_case else 4 if combine else 6  # (the contract's Python oracles are what a combine case costs: run_reads' budget; C4: 5, 1, 33 resources twice)
    unread_write = False   # an accepted write no read has followed yet
    last_check_deep = None  # did the previous Check round hold an item that ends at the depth limit
    todo = []
    t0 = time.time()

    def check_round(n):
        qs = [rand_query(rr, names, combine) for _ in range(n)]
        if recycle and n >= 7:  # objects first named by this stream, on both sides of an item
            fp, fu = reads.first_seen_in_stream("pod"), [u for u in reads.names_of("user") if u.startswith("newcomer")]
            if fp: qs[1] = ("pod", rr.choice(fp), "view", "user", rr.choice(users), "")
            if fu: qs[2] = ("pod", rr.choice(pods), "view", "user", rr.choice(fu), "")
            stats["check_first_seen_items"] += bool(fp) + bool(fu)
        want = {q: tuple(o.check(*q)) for q in set(qs)}
        return qs, [want[q] for q in qs]

    for step in range(steps):
        rec.step = step
        if clock is not None and rng.random() < 0.25:  # (every rank sets its engine's clock; the probe batch is a Check step of the script)
            _d, _gone, want = clock.move(step, live)
            reads.clock_moves += 1
            script.append(("clock", step, clock.now))
            script.append(("check", step, list(clock.probe), want, "probe"))
            accepted = False
        elif rng.random() < 0.9:
            accepted = write_batch(rng, step, rand_tuple, o, rec, live, 25, stats, clock)
        else:
            accepted = filter_delete(rng, step, names, combine, o, rec, live, stats, clock) > 0
        if accepted:
            reads.version += 1
            stats["writes_accepted"] += 1
            unread_write = True
        if rr.random() < read_share:
            if not todo:
                todo = ["check", "lookup"] + (["subjects"] if (reads.subject_targets if depth_case else stats["rounds_subjects"]) < subject_rounds else [])
                rr.shuffle(todo)
            kind = todo.pop()
            reads.round_no += 1
            done = True
            t1 = time.time()
            if kind == "check":
                qs, want = check_round(SHARD_CHECK_SIZES[stats["rounds_check"] % len(SHARD_CHECK_SIZES)])
                deep = sum(w[1] == orc.ERR_DEPTH for w in want)
                stats["check_items"] += len(qs)
                stats["check_depth_items"] += deep
                stats["check_has_items"] += sum(w == (2, 0) for w in want)
                stats["check_outruns_expected"] += bool(deep) and last_check_deep is False  # the level loop's burst was sized by a shallower batch
                last_check_deep = bool(deep)
                script.append(("check", step, qs, want))
            elif kind == "lookup":
                rt, pm = rr.choice(lookup_perms)
                subs = rr.sample(reads.names_of("user"), (1, 4)[stats["rounds_lookup"] % 2])
                want = [reads.lookup_expected(rt, pm, "user", u) for u in subs]
                after = []
                if any(w[0] == "err" for w in want):
                    stats["lookup_calls_failed"] += 1
                    ok = [(u, w) for u, w in zip(subs, want) if w[0] == "ok"]
                    after = [("lookup", [u], [w]) for u, w in ok] or [("check",) + check_round(7)]
                stats["lookup_calls"] += 1
                stats["lookup_rows"] += len(subs)
                stats["lookup_rows_nonempty"] += sum(w[0] == "ok" and bool(w[1]) for w in want)
                script.append(("lookup", step, rt, pm, subs, want, after))
            else:
                mark = len(reads.asked)
                done = reads.round_subjects(step)
                if done and not depth_case:  # ... and a resource the generator knows that has lost, or never had, relationships of its own
                    rt, pm = reads.asked[mark][:2]
                    bare = sorted(set({"pod": pods, "namespace": nss, "group": groups}[rt]) - set(reads.resources_with_relationships(rt)))
                    if bare:
                        reads.subjects_expected(rt, pm, "user", "", [rr.choice(bare)], {})
                        stats["subj_no_relationships"] += 1
                if done and depth_case and not stats["subj_answered_over_arrow"]:
                    # the targets that answer there have no Check that errs, so no cyclic group behind them: what crosses shards in an answered call is a namespace's
                    # viewer relation with its groups' members (monotone: users beyond the depth limit are left out silently, the call answers)
                    with_groups = sorted({r[1] for r in reads.rels() if r[0] == "namespace" and r[2] == "viewer" and r[3] == "group"})
                    if with_groups:
                        reads.subjects_expected("namespace", "viewer", "user", "", [rr.choice(with_groups)], {})
                asked = reads.asked[mark:]
                for _rt, _pm, _st, _srel, _rids, want in asked:
                    failed = any(w == "DEPTH" for w in want)
                    stats["subj_calls"] += 1
                    stats["subj_calls_failed"] += failed
                    stats["subj_calls_answered"] += not failed
                    # (an answered call that crosses shards at every world the cases use: a pod's permission through pod#namespace, a namespace's through its groups)
                    stats["subj_answered_over_arrow"] += not failed and any(r[1] in _rids and ((_rt, r[0], r[2]) == ("pod", "pod", "namespace") and _pm != "edit" or
                                                                                           (_rt, r[0], r[2], r[3]) == ("namespace", "namespace", "viewer", "group")) for r in reads.rels())
                    stats["subj_wildcard_excluded"] += sum(w != "DEPTH" and w[1] and bool(w[2]) for w in want)
                if done:
                    script.append(("subjects", step, asked))
            stats["seconds_" + kind] = round(stats.get("seconds_" + kind, 0.0) + time.time() - t1, 2)
            stats["rounds"] += 1
            stats["rounds_" + kind] += bool(done)
            stats["skipped"] += not done
            if done and clock is not None and clock.moved_last:  # (a read round behind a clock move with no accepted write in between)
                stats["reads_behind_clock_" + kind] += 1
            if done and unread_write:
                stats["writes_read_before_next"] += 1
                unread_write = False
        elif accepted:
            unread_write = False  # (the next write comes before a read)
        if verbose and step % 10 == 9:
            print(f"step {step + 1}/{steps}: {stats}, {len(live)} relationships, {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
    stats["seconds_script"] = round(time.time() - t0, 1)
    return dict(schema_text=schema_text, combine=combine, init=init, steps=script, stats=stats, now0=CLOCK_START if expiring else None)


def step_names(st):
    """the (type, name) pairs a read step interns, in the order every rank interns them"""
    def of_items(qs):
        for rt, rid, _pm, s, sid, _srel in qs:
            yield (rt, rid)
            yield (s, sid)

    if st[0] == "check":
        yield from of_items(st[2])
    elif st[0] == "lookup":
        for u in st[4]:
            yield ("user", u)
        for f in st[6]:
            if f[0] == "check":
                yield from of_items(f[1])
    elif st[0] == "subjects":
        for rt, _pm, _st, _srel, rids, _want in st[2]:
            for r in rids:
                yield (rt, r)


def sharded_dry_engines(script, world: int, recycle: bool, compact_early: bool) -> list:
    """The script's writes on one store-only engine per rank (acl_shard_configure(rank, world)), one after the other; at every read step the rank's host snapshot is
    brought up to date the way a read would and verified against the store.  -> per rank {"owns", 0: rebuilt, 1: patched, 2: current, "adopted", "dropped"}."""
    out = []
    for rank in range(world):
        e = open_engine(script["schema_text"], recycle, False, store_only=True)
        try:
            e._check(e._L.acl_shard_configure(e._h, rank, world))
            if script.get("now0"):
                e.set_now(script["now0"])
            for st in script["init"]:
                e.write(st[2])
            e.selfcheck_snapshot_code()  # (the first build is not counted)
            codes = {"owns": [t for t in ("group", "namespace", "pod") if e._L.acl_shard_of_type(e._h, e.type_id(t)) == rank], 0: 0, 1: 0, 2: 0, "adopted": 0, "dropped": 0}
            pending, nwrites, started = None, 0, 0
            every = 8 if compact_early else 30  # (the engine compacts in the background on these graphs without ACL_COMPACTION_SLACK=0 too, only less often)
            for st in script["steps"]:
                if st[0] in ("write", "filter"):
                    sharded_apply_write(e, st)
                    nwrites += 1
                    # a background compaction's two halves around the writes in between, as run_patcher drives them: built from a copy-on-write view behind
                    # every `every`-th write, adopted 0, 1, ... 5 writes later with the writes since replayed onto it
                    if pending is None and nwrites % every == every // 2:
                        e.selfcheck_compaction(0)
                        pending = started % 6
                        started += 1
                    elif pending is not None:
                        if pending == 0:
                            codes["adopted" if e.selfcheck_compaction(1) else "dropped"] += 1  # (phase 1 verifies the adopted snapshot against the store)
                            pending = None
                        else:
                            pending -= 1
                elif st[0] == "clock":  # (the rank's patched snapshot is verified behind the move itself, and again at the read step that follows)
                    e.set_now(st[2])
                    codes[e.selfcheck_snapshot_code()] += 1
                else:
                    for t, n in dict.fromkeys(step_names(st)):
                        e.intern(t, n)
                    codes[e.selfcheck_snapshot_code()] += 1  # (raises when the snapshot does not describe the store)
            codes["ids_recycled"] = int(e.stats().get("ids_recycled", 0))
            out.append(codes)
        finally:
            e.close()
    return out


def sharded_apply_write(e, st):
    """one write step of the script on an engine -> None, or what differs from the oracle's outcome"""
    import aclgpu
    if st[0] == "filter":
        n = e.delete_by_filter(**st[2])
        return None if n == st[3] else (st[2], n, st[3])
    code = None
    try:
        e.write(st[2])
    except aclgpu.AclError as x:
        code = x.code
    return None if code == st[3] else (st[2][:3], code, st[3])


def sharded_replay(script, host_driven: bool):
    """-> fn(ShardedEngine) for sharded.run_logical_shards: one rank's replay of the script.  A wrong answer is recorded as (step, rank, kind, request, got, want) and the
    rank goes on; it returns its records, one line of the stats struct per native call, a digest of the ids it interned per read step, and its engine's stats."""
    import zlib
    import numpy as np
    import aclgpu

    def names_of_row(e, t, row):
        return set(e.bitmap_names(t, row.cpu().numpy().view(np.uint32)))

    def replay(se):
        e, rank = se.shard.e, se.shard.rank
        bad, calls, digests, refusals = [], [], [], []
        behind_clock = [False]  # a clock move and no accepted write since: the calls noted meanwhile carry it
        tid = {t: e.type_id(t) for t in ("user", "group", "namespace", "pod")}
        rel = {}

        def rel_id(t, m):
            if (t, m) not in rel:
                rel[(t, m)] = e.relation_id(t, m)
            return rel[(t, m)]

        def items_of(qs, ids):
            out = np.zeros(len(qs), dtype=aclgpu.ITEM_DTYPE)
            for i, (rt, rid, pm, s, sid, srel) in enumerate(qs):
                out[i] = (tid[rt], rel_id(rt, pm), ids[(rt, rid)], tid[s], rel_id(s, srel) if srel else aclgpu.NO_RELATION, ids[(s, sid)])
            return out

        def note(step, kind, follows_write, s):
            calls.append((step, kind, follows_write, s["levels"], s["retries"], s["entries_exchanged"], s["host_syncs"], s["export_capacity"], behind_clock[0]))

        def check(step, qs, want, ids, follows_write, kind="check"):
            items = items_of(qs, ids)
            p, er, s = se.check_bulk_ids_native(items)
            note(step, kind, follows_write, s)
            got = list(zip(p.cpu().tolist(), er.cpu().tolist()))
            diff = [i for i in range(len(qs)) if got[i] != tuple(want[i])]
            if diff:
                bad.append((step, rank, kind + " native", (qs[diff[0]], f"item {diff[0]} of {len(qs)}, {len(diff)} differ"), got[diff[0]], want[diff[0]]))
            if host_driven:
                p2, er2 = se.check_bulk_ids(items)
                got2 = list(zip(p2.cpu().tolist(), er2.cpu().tolist()))
                diff = [i for i in range(len(qs)) if got2[i] != tuple(want[i])]
                if diff:
                    bad.append((step, rank, kind + " host-driven", (qs[diff[0]], f"item {diff[0]} of {len(qs)}, {len(diff)} differ"), got2[diff[0]], want[diff[0]]))
                if got2 != got:
                    i = next(i for i in range(len(qs)) if got[i] != got2[i])
                    bad.append((step, rank, kind + ": the routes differ", qs[i], got2[i], got[i]))
            elif not any(r[0] == "check" for r in refusals):  # a schema with `-` / `&` / .all(): the step protocol refuses it, on every rank before any collective
                try:
                    se.check_bulk_ids(items)
                    refusals.append(("check", None))
                except aclgpu.AclError as x:
                    refusals.append(("check", x.code))

        def lookup(step, rt, pm, subs, want, ids, follows_write, kind="lookup"):
            sids = [ids[("user", u)] for u in subs]
            fails = next((w[1] for w in want if w[0] == "err"), None)
            routes = [("native", lambda: se.lookup_ids_batch_native(rt, pm, "user", "", sids))]
            if host_driven:
                routes.append(("host-driven", lambda: (se.lookup_ids_batch(rt, pm, "user", "", sids), None)))
            elif not any(r[0] == "lookup" for r in refusals):
                try:
                    se.lookup_ids_batch(rt, pm, "user", "", sids)
                    refusals.append(("lookup", None))
                except aclgpu.AclError as x:
                    refusals.append(("lookup", x.code))
            for route, call in routes:
                try:
                    bm, s = call()
                except aclgpu.AclError as x:  # a candidate's Check erred: every rank fails the call, at the same point
                    if x.code != fails:
                        bad.append((step, rank, f"{kind} {route}", (rt, pm, subs), ("err", x.code), [w[0] for w in want]))
                    continue
                if s is not None:
                    note(step, kind, follows_write, s)
                if fails is not None:
                    bad.append((step, rank, f"{kind} {route}", (rt, pm, subs), "answered", ("err", fails)))
                    continue
                for i, (u, w) in enumerate(zip(subs, want)):
                    got = names_of_row(e, rt, bm[i])
                    if got != w[1]:
                        bad.append((step, rank, f"{kind} {route}", (rt, pm, u), f"engine only {sorted(got - w[1])[:5]}", f"oracle only {sorted(w[1] - got)[:5]}"))

        def subjects(step, req, ids, follows_write):
            rt, pm, s_t, srel, rids, want = req
            fails = any(w == "DEPTH" for w in want)
            try:
                bm, flags, ex, s = se.lookup_subjects_ids_batch_native(rt, pm, s_t, srel, [ids[(rt, r)] for r in rids], want_excluded=True)
            except aclgpu.AclError as x:
                if not (fails and x.code == aclgpu.ERR_DEPTH):
                    bad.append((step, rank, "subjects", (rt, pm, s_t, srel, rids[:3]), ("err", x.code), "DEPTH" if fails else "an answer"))
                return
            note(step, "subjects", follows_write, s)
            if fails:
                bad.append((step, rank, "subjects", (rt, pm, s_t, srel, [r for r, w in zip(rids, want) if w == "DEPTH"][:3]), "answered", "DEPTH"))
                return
            for i, (r, (wids, wild, wex)) in enumerate(zip(rids, want)):
                got = names_of_row(e, s_t, bm[i])
                if got != wids:
                    bad.append((step, rank, "subjects", (rt, r, pm, s_t, srel), f"engine only {sorted(got - wids)[:5]}", f"contract only {sorted(wids - got)[:5]}"))
                if bool(flags[i] & 1) != wild:
                    bad.append((step, rank, "subjects wildcard flag", (rt, r, pm, s_t, srel), int(flags[i]), wild))
                if wild:
                    gex = names_of_row(e, s_t, ex[i])
                    if gex != wex:
                        bad.append((step, rank, "subjects excluded", (rt, r, pm, s_t, srel), sorted(gex ^ wex)[:5], "(symmetric difference)"))

        if script.get("now0"):
            e.set_now(script["now0"])
        for st in script["init"]:
            e.write(st[2])
        follows_write = False  # (the first read follows the starting graph's load: a built snapshot, not a patched one)
        for st in script["steps"]:
            if st[0] in ("write", "filter"):
                d = sharded_apply_write(e, st)
                if d is not None:
                    bad.append((st[1], rank, st[0]) + d)
                accepted = st[3] is None if st[0] == "write" else st[3] > 0
                follows_write = follows_write or accepted
                behind_clock[0] = behind_clock[0] and not accepted
                continue
            if st[0] == "clock":  # (no write: the next read of this rank patches every relationship whose liveness changed)
                e.set_now(st[2])
                behind_clock[0] = True
                continue
            ids = {}
            for k in step_names(st):
                if k not in ids:
                    ids[k] = e.intern(*k)
            digests.append(zlib.crc32(np.asarray(list(ids.values()), dtype=np.uint32).tobytes()))
            if st[0] == "check":
                check(st[1], st[2], st[3], ids, follows_write)
            elif st[0] == "lookup":
                lookup(st[1], st[2], st[3], st[4], st[5], ids, follows_write)
                for f in st[6]:
                    if f[0] == "check":
                        check(st[1], f[1], f[2], ids, False, kind="check behind a failed lookup")
                    else:
                        lookup(st[1], st[2], st[3], f[1], f[2], ids, False, kind="lookup behind a failed lookup")
            else:
                for req in st[2]:
                    subjects(st[1], req, ids, follows_write)
            follows_write = False
            if not (st[0] == "check" and len(st) > 4):  # (the probe batch behind a move leaves the mark for the step's own read round)
                behind_clock[0] = False
        est = e.stats()
        return dict(rank=rank, bad=bad, calls=calls, digests=digests, refusals=refusals, owns=[t for t in ("group", "namespace", "pod") if se.shard.owner_of_type(t) == rank],
                    **{k: int(est[k]) for k in ("snapshot_builds", "snapshot_patches", "snapshot_compactions", "ids_recycled", "overflow_retries") if k in est})

    return replay


def run_sharded(seed: int, steps: int, world: int, schema: str = "c4", acyclic: bool = False, recycle: bool = False, compact_early: bool = False, universe: int = 1,
                engine: bool = True, verbose: bool = True, depth_case: bool = False, read_share: float = 0.75, exchange: str = "allgather", xcap: int = 0,
                expiring: bool = False, probe: int = 200) -> dict:
    """The read campaign's kind of write stream under the loops of the type-hash sharded graph.  Phase 1 (sharded_script) computes, with the oracles alone, the script
    of writes and reads with their expected outcomes; phase 2 replays it on `world` logical shards of one GPU (sharded.run_logical_shards: one Engine per rank, a
    replicated store, one thread each), every rank holding every answer to the script by name:
      a. Check batches of 1, 7, 64, 900 and 3000 items through acl_shard_check_bulk and, on the same step, the host-driven step protocol (`exchange`), route against route;
      b. LookupResources of 1 and 4 subjects through acl_shard_lookup_bulk and the host-driven protocol, or the failure code on every rank and a correct next call;
      c. LookupSubjects of 1, 5 and 33 resources with the excluded rows (acl_shard_subjects_bulk), user and group#member subjects, or ACL_ERR_DEPTH on every rank;
      d. levels / retries / entries_exchanged / host_syncs / export_capacity of every native call, for the conditions on the burst hints and on grow-and-redo.
    The host-driven protocol refuses schemas with `-` / `&` / .all() (ShardCall::begin): there the native loops alone answer and the refusal's code is recorded once.
    engine=False: phase 1, and the script's writes on one store-only engine per rank whose patched host snapshot is verified against the store at every read step.
    xcap: ACL_SHARD_XCAP around the replay (a first export block of that many entries: grow-and-redo).  -> stats; raises AssertionError on the first record."""
    script = sharded_script(seed, steps, schema, acyclic, recycle, universe, depth_case, read_share, verbose, expiring, probe)
    stats = script["stats"]
    t0 = time.time()
    if not engine:
        stats["dry_ranks"] = sharded_dry_engines(script, world, recycle, compact_early)
        stats["seconds_dry_engines"] = round(time.time() - t0, 1)
        return stats
    import aclgpu
    from aclgpu import sharded
    env = {"ACL_ID_QUARANTINE_MS": "0" if recycle else None, "ACL_COMPACTION_SLACK": "0" if compact_early else None, "ACL_SHARD_XCAP": str(xcap) if xcap else None}
    before = {k: os.environ.get(k) for k in env}
    engines = []

    def make(rank, nshards):  # (open_engine's environment, set once around every rank's engine: the ranks are threads of this process)
        # (a frontier of 2^20 entries in place of the default 2^25: eight engines share the device, and a batch that outgrows it grows it under the reads)
        e = aclgpu.Engine(script["schema_text"], contexts=1, frontier_entries=1 << 20)
        engines.append(e)
        return sharded.GpuShard(e, rank, nshards)

    fn = sharded_replay(script, host_driven=not script["combine"])
    fn.exchange = exchange
    try:
        for k, v in env.items():
            if v is not None:
                os.environ[k] = v
        outs = sharded.run_logical_shards(world, make, fn)
    finally:
        for k, v in before.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        for e in engines:
            e.close()
    stats["seconds_replay"] = round(time.time() - t0, 1)
    bad = [b for out in outs for b in out["bad"]]
    for out in outs[1:]:  # a replicated store: every rank gave every name the id rank 0 gave it (recycled ones too)
        d = next((i for i, (a, b) in enumerate(zip(outs[0]["digests"], out["digests"])) if a != b), None)
        if d is not None:
            bad.append((f"read step {d}", out["rank"], "interned ids differ from rank 0's", None, out["digests"][d], outs[0]["digests"][d]))
    stats["ranks"] = [{k: v for k, v in out.items() if k not in ("bad", "calls", "digests")} for out in outs]
    stats["calls"] = outs[0]["calls"]  # (step, kind, follows a write, levels, retries, entries_exchanged, host_syncs, export_capacity, behind a clock move) of rank 0's native calls
    stats["calls_equal_on_every_rank"] = all([c[:5] + c[7:] for c in out["calls"]] == [c[:5] + c[7:] for c in outs[0]["calls"]] for out in outs)
    if bad:
        bad.sort(key=lambda b: (b[0] if isinstance(b[0], int) else 1 << 30, b[1]))
        raise AssertionError(f"{len(bad)} records; the first: step {bad[0][0]}, rank {bad[0][1]}, {bad[0][2]}: request {bad[0][3]}: got {bad[0][4]}, want {bad[0][5]}")
    return stats


def run_expiry(seed: int, steps: int, verbose: bool = True) -> dict:
    """The reference's own schema (pkg/spicedb/bootstrap.yaml) under the dual write's shapes: lock tuples created behind MUST_NOT_MATCH and deleted
    again (workflow.go:392-462), idempotency keys that EXPIRE (activity.go:81-102), payload relationships -- while the clock moves forwards in
    random steps (seconds to days: keys run out in between, expired ones are collected after 24 h).  After every step a batch of checks on live,
    expired and never-written keys, locks and payloads, and ReadRelationships of the expiring class, must equal the oracle's."""
    import json

    import aclgpu
    from oracle import orc
    from aclgpu.text import parse_relationship
    from oracle.orc import parse_rel

    rng = random.Random(seed)
    b = json.load(open(os.path.join(ROOT, "tests", "golden", "bootstrap.json")))
    e = aclgpu.Engine(b["schema"], "\n".join(b["relationships"]))
    o = orc.Oracle(b["schema"])
    o.write([(orc.OP_TOUCH, r) for r in b["relationships"]])
    now = 1_700_000_000
    e.set_now(now)
    o.set_now(now)
    wfs = [f"wf{i}" for i in range(40)]
    acts = [f"act{i:x}" for i in range(120)]
    locks = [f"lk{i:x}" for i in range(30)]
    users = [f"u{i}" for i in range(20)]
    nss = [f"ns{i}" for i in range(12)]
    stats = {"writes": 0, "write_errors": 0, "clock_moves": 0, "checks": 0, "reads": 0, "subject_lookups": 0, "subject_rows_nonempty": 0, "live_keys_explained": 0,
             "expired_keys_explained": 0}
    written_keys = set()
    OPS = {aclgpu.OP_TOUCH: orc.OP_TOUCH, aclgpu.OP_CREATE: orc.OP_CREATE, aclgpu.OP_DELETE: orc.OP_DELETE}
    for step in range(steps):
        r = rng.random()
        if r < 0.5:
            ups, pre = [], []
            k = rng.random()
            if k < 0.45:    # the pessimistic dual write's first request: payload + lock CREATE behind MUST_NOT_MATCH + an expiring idempotency key
                lk, wf = rng.choice(locks), rng.choice(wfs)
                pre = [(aclgpu.PRE_MUST_NOT_MATCH, dict(rtype="lock", rid=lk, rel="workflow"))]
                ups = [(aclgpu.OP_TOUCH, f"namespace:{rng.choice(nss)}#creator@user:{rng.choice(users)}"),
                       (aclgpu.OP_CREATE, f"lock:{lk}#workflow@workflow:{wf}"),
                       (aclgpu.OP_TOUCH, f"workflow:{wf}#idempotency_key@activity:{rng.choice(acts)}", now + rng.choice([1, 5, 60, 3600, 86400, 200000]))]
            elif k < 0.8:   # ... and its second: the lock goes away
                ups = [(aclgpu.OP_DELETE, f"lock:{rng.choice(locks)}#workflow@workflow:{rng.choice(wfs)}")]
            else:           # keys rewritten with a new expiry, or none
                ups = [(aclgpu.OP_TOUCH, f"workflow:{rng.choice(wfs)}#idempotency_key@activity:{rng.choice(acts)}", rng.choice([0, now + 2, now + 30, now - 5]))
                       for _ in range(rng.randrange(1, 6))]
                ups = list({u[1]: u for u in ups}.values())
            eo = ee = None
            try:
                o.write([(OPS[u[0]],) + tuple(u[1:]) for u in ups], [({aclgpu.PRE_MUST_NOT_MATCH: orc.PRE_MUST_NOT_MATCH}[p[0]], p[1]) for p in pre])
            except orc.OracleError as x:
                eo = x.code
            try:
                e.write(ups, pre)
            except aclgpu.AclError as x:
                ee = x.code
            assert eo == ee, f"step {step}: write outcome differs: oracle {eo}, engine {ee}: {ups} {pre}"
            stats["writes"] += 1
            stats["write_errors"] += eo is not None
            if eo is None:  # (the keys this stream has written, for the reads below: an expired one is one of these that the oracle no longer reads)
                written_keys.update(parse_rel(u[1])[:6] for u in ups if u[0] != aclgpu.OP_DELETE and u[1].startswith("workflow:"))
        elif r < 0.7:
            now += rng.choice([1, 1, 3, 10, 61, 3601, 50000, 90000])
            e.set_now(now)
            o.set_now(now)
            stats["clock_moves"] += 1
        qs = [("workflow", rng.choice(wfs), "idempotency_key", "activity", rng.choice(acts), "") for _ in range(150)] + \
             [("lock", rng.choice(locks), "workflow", "workflow", rng.choice(wfs), "") for _ in range(40)] + \
             [("namespace", rng.choice(nss), rng.choice(["view", "edit", "admin", "no_one_at_all"]), "user", rng.choice(users + ["rakis"]), "") for _ in range(40)] + \
             [("namespace", "spicedb-kubeapi-proxy", "view", "user", "rakis", "")]
        perms, errs = e.check_bulk(qs)
        for i, q in enumerate(qs):
            assert (perms[i], errs[i]) == tuple(o.check(*q)), f"step {step} (now {now}): check {q}: engine {(perms[i], errs[i])}, oracle {o.check(*q)}"
        stats["checks"] += len(qs)
        if step % 5 == 0:  # ReadRelationships of the expiring class (activity.go:107-149 reads the keys back): expired ones are gone on both sides
            a, b2 = sorted(e.read(rtype="workflow")), sorted(o.read(rtype="workflow"))
            assert [x[:6] for x in a] == [x[:6] for x in b2], f"step {step} (now {now}): workflow relationships differ: {set(a) ^ set(b2)}"
            stats["reads"] += 1
        # ---- the other read paths on the same snapshot, without a draw from rng: LookupSubjects of three workflows' keys, Explain of a live and of an expired key
        held = {}
        for x in o.read(rtype="workflow"):
            held.setdefault(x[1], set()).add(x[4])
        for k in range(3):
            wf = wfs[(3 * step + k) % len(wfs)]
            got = e.lookup_subjects("workflow", wf, "idempotency_key", "activity")
            assert got == (held.get(wf, set()), False, set()), f"step {step} (now {now}): LookupSubjects of workflow:{wf}#idempotency_key: engine {got}, the oracle reads {held.get(wf, set())}"
            stats["subject_lookups"] += 1
            stats["subject_rows_nonempty"] += bool(held.get(wf))
        live_keys = sorted((wf, a) for wf, acts_ in held.items() for a in acts_)
        if live_keys:
            wf, a = live_keys[step % len(live_keys)]
            got = e.explain("workflow", wf, "idempotency_key", "activity", a)
            assert got[:3] == (2, 0, aclgpu.EXPLAIN_WITNESS) and [tuple(parse_relationship(ln))[:6] for ln in got[3]] == [("workflow", wf, "idempotency_key", "activity", a, "")], f"step {step} (now {now}): Explain of the live key {wf}/{a}: {got}"
            stats["live_keys_explained"] += 1
        expired = sorted((r6[1], r6[4]) for r6 in written_keys if r6[4] not in held.get(r6[1], ()))
        if expired:
            wf, a = expired[step % len(expired)]
            got = e.explain("workflow", wf, "idempotency_key", "activity", a)
            assert got == (1, 0, 0, []) and tuple(o.check("workflow", wf, "idempotency_key", "activity", a)) == (1, 0), f"step {step} (now {now}): Explain of the expired key {wf}/{a}: {got}"
            stats["expired_keys_explained"] += 1
        if verbose and step % 100 == 99:
            print(f"step {step + 1}/{steps}: {stats}, now +{now - 1_700_000_000} s", file=sys.stderr, flush=True)
    st = e.stats()
    stats.update({k: int(st[k]) for k in ("snapshot_builds", "snapshot_patches", "snapshot_compactions") if k in st})
    e.close()
    return stats


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--burst", type=int, default=25, help="updates per write, at most (<= 1000: the reference's limit, spicedb.go:35)")
    ap.add_argument("--compact-early", action="store_true", help="ACL_COMPACTION_SLACK=0: background compactions (and their adoption with the writes since replayed) happen on this small graph too")
    ap.add_argument("--patcher", action="store_true", help="no GPU: a store-only engine whose host snapshot is verified against the store after every write")
    ap.add_argument("--expiry", action="store_true", help="the other campaign: the reference's bootstrap schema, dual-write shapes, expiring idempotency keys, a moving clock")
    ap.add_argument("--schema", choices=["c4", "combine"], default="c4", help="combine: the C4 schema with exclusions, intersections, wildcards and a non-monotone userset subject")
    ap.add_argument("--recycle", action="store_true", help="ACL_ID_QUARANTINE_MS=0 and a stream of never-seen object names in the writes: ids of objects that lost their last relationship are taken over under the reads")
    ap.add_argument("--acyclic", action="store_true", help="group nesting without cycles: one-user CheckBulkPermissions calls take the reverse walk once the depth sweep has run")
    ap.add_argument("--expiring", action="store_true", help="the schema with `with expiration` on its relations (SCHEMA_C4_EXPIRING / SCHEMA_COMBINE_EXPIRING), writes with an expiry and a clock that moves forwards and back between the writes; with --reads, --patcher, --sharded W and --dry too")
    ap.add_argument("--reads", action="store_true", help="the read campaign (run_reads): LookupSubjects, Explain witness / proof / denial, multi-target lookups and cursors held across the writes")
    ap.add_argument("--dry", action="store_true", help="with --reads: the oracle's half alone, no engine and no GPU")
    ap.add_argument("--depth-case", action="store_true", help="with --reads: LookupSubjects and multi-target lookups only, four LookupSubjects targets in all (cyclic combine graphs)")
    ap.add_argument("--universe", type=int, default=1, help="scale of the object universe (x 160 users, 48 groups, 8 namespaces, 240 pods)")
    ap.add_argument("--sharded", type=int, default=0, metavar="W", help="the sharded campaign (run_sharded): the stream's script replayed on W logical shards of one GPU; with --dry on W store-only engines")
    ap.add_argument("--exchange", choices=["allgather", "alltoall"], default="allgather", help="with --sharded: how the host-driven protocol's Check frontiers cross shards")
    ap.add_argument("--xcap", type=int, default=0, help="with --sharded: ACL_SHARD_XCAP around the replay (a first export block of that many entries)")
    ap.add_argument("--read-share", type=float, default=0.75, help="with --sharded: the share of steps with a read round behind the write")
    a = ap.parse_args()
    try:
        print(run_sharded(a.seed, a.steps, a.sharded, schema=a.schema, acyclic=a.acyclic, recycle=a.recycle, compact_early=a.compact_early, universe=a.universe,
                          engine=not a.dry, depth_case=a.depth_case, read_share=a.read_share, exchange=a.exchange, xcap=a.xcap, expiring=a.expiring) if a.sharded
              else run_patcher(a.seed, a.steps, a.universe, a.burst, schema=a.schema, expiring=a.expiring) if a.patcher else run_expiry(a.seed, a.steps) if a.expiry
              else run_reads(a.seed, a.steps, schema=a.schema, acyclic=a.acyclic, recycle=a.recycle, compact_early=a.compact_early, universe=a.universe, engine=not a.dry,
                             depth_case=a.depth_case, expiring=a.expiring) if a.reads
              else run(a.seed, a.steps, burst=a.burst, universe=a.universe, compact_early=a.compact_early, schema=a.schema, recycle=a.recycle, acyclic=a.acyclic,
                       expiring=a.expiring, engine=not a.dry))
    except AssertionError as x:
        print("MISMATCH:", x)
        sys.exit(1)

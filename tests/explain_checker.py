"""The one checker every Explain witness is held to (tests/test_explain_gpu.py; its own behaviour is checked on the CPU by tests/test_explain_cpu.py).

A witness is a list of relationships (rtype, rid, rel, stype, sid, srel) -- a wildcard hop names the subject id "*".  The contract:
  - at most 50 of them, every one in the test's own relationship set;
  - they chain: the first hop's resource is the item's resource object, each hop's subject object is the next hop's resource object, and the
    last hop names the item's subject (or the subject type's `*`); an item whose subject carries a relation may end at that object's own state;
  - the hops ALONE, loaded into an empty store under the same schema, make both oracles' Check of the item answer HAS -- each hop written with the expiry
    it has in the store (`expires`: {relationship: expires_at}) and both oracles at the store's clock (`now`), so a hop that has run out grants nothing."""
from oracle import orc
from oracle.pyoracle import HAS, PyOracle

MAX_HOPS = 50


def replay(schema, item, hops, expires=None, now=0):
    """(Python oracle's answer, C oracle's (permissionship, error)) for `item` on a store that holds only `hops`, at clock `now`"""
    py, c = PyOracle(schema), orc.Oracle(schema)
    py.now = now
    c.set_now(now)
    at = expires or {}
    for h in hops:
        py.touch(*h[:6], expires=at.get(tuple(h[:6]), 0))
    if hops:
        c.write([(orc.OP_TOUCH, tuple(h[:6]), at.get(tuple(h[:6]), 0)) for h in hops])
    return py.check(*item), c.check(*item)


def check_witness(schema, relationships, item, hops, replay_it=True, expires=None, now=0):
    """item: (rt, rid, perm, st, sid, srel); relationships: a set of 6-tuples, or a predicate over one; expires, now: see replay()"""
    rt, rid, _perm, st, sid, srel = item
    has = relationships if callable(relationships) else (lambda h: h in relationships)
    assert len(hops) <= MAX_HOPS, len(hops)
    for h in hops:
        assert has(tuple(h[:6])), f"hop {h} is not a stored relationship"
    at = (rt, rid)
    for h in hops:
        assert (h[0], h[1]) == at, f"hop {h} does not start at {at}: {hops}"
        at = (h[3], h[4])
    if srel:
        assert at == (st, sid), f"the chain ends at {at}, not at the subject's object: {hops}"
    else:
        assert hops, "a plain subject is never granted by zero hops"
        assert hops[-1][3:6] in ((st, sid, ""), (st, "*", "")), f"the last hop does not name the subject: {hops}"
    if replay_it:
        p, c = replay(schema, item, hops, expires, now)
        assert p == HAS, f"Python oracle: {p} for {item} on {hops}"
        assert c == (2, 0), f"C oracle: {c} for {item} on {hops}"

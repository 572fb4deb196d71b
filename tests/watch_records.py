"""What a watch set's poll must report, from rows that the oracles define: shared by tests/test_watch_set_gpu.py (resource direction: a watcher is a subject,
its row the resources it holds the permission on), tests/test_subject_watch_gpu.py (subject direction: a watcher is a resource, its row the subjects that
hold the permission on it) and the `watch` rounds of tools/fuzz_gpu.py's read campaign.

A record is (watcher, id, gained[, reserved]); a poll's records are ordered by (watcher, id), so whole lists are compared."""


def expected_records(held, after, id_of, reserved_of=None):
    """held: {watcher: the row (a set of names) at its last poll, or None: whatever it holds now}; after: {watcher: the row now}; id_of(name) -> the engine's
    id of a name in a row (never None); reserved_of(id) -> the record's fourth field (None: three-field records).  -> the records of the next poll"""
    recs = []
    for w in sorted(after):
        before = after[w] if held[w] is None else held[w]
        ch = [(id_of(n), 1) for n in after[w] - before] + [(id_of(n), 0) for n in before - after[w]]
        assert all(i is not None for i, _g in ch), (w, "a changed name has no id")
        recs += [(w, i, g) if reserved_of is None else (w, i, g, reserved_of(i)) for i, g in sorted(ch)]
    return recs


def records_of(recs, reserved=False):
    """a poll's records (WATCH_CHANGE_DTYPE) as tuples"""
    if reserved:
        return [(int(r["watcher"]), int(r["resource_id"]), int(r["gained"]), int(r["reserved"])) for r in recs]
    return [(int(r["watcher"]), int(r["resource_id"]), int(r["gained"])) for r in recs]

"""acl_lookup_resources_multi / acl_access_review without a GPU: arguments are validated before the engine's mode is looked at (a store-only engine answers
ACL_ERR_UNAVAILABLE only for a call that is otherwise in order), the Python wrappers lay the rows out as the header says, and the statistics end in the
two new fields."""
import ctypes as C

import numpy as np
import pytest

SCHEMA = """definition user {}
definition group { relation member: user | group#member }
definition doc { relation viewer: user | group#member
 relation owner: user
 permission view = viewer + owner }"""


@pytest.fixture(scope="module")
def eng(aclgpu_lib):
    import aclgpu
    e = aclgpu.Engine(SCHEMA, store_only=True)
    e.touch(*[("doc", f"d{i}", "viewer", "user", "u", "") for i in range(40)])  # 40 docs: two words per doc row
    e.touch(("group", "g", "member", "user", "u", ""))
    yield e
    e.close()


def raw_call(e, targets, row_words, n=1, stype="user", srel=-1, null=()):
    from aclgpu._lib import Target
    T = len(targets)
    tg = (Target * max(1, T))(*[Target(rt, pm) for rt, pm in targets])
    sids = np.zeros(max(1, n), dtype=np.uint32)
    words = np.asarray(list(row_words) + [0], dtype=np.uintp)
    buf = np.full((max(1, n), max(1, int(sum(row_words)))), 0xFFFFFFFF, dtype=np.uint32)
    cnt = np.full((max(1, n), max(1, T)), 7, dtype=np.uint64)
    rc = e._L.acl_lookup_resources_multi(e._h, None if "targets" in null else tg, T, e.type_id(stype), srel, None if "sids" in null else sids.ctypes.data, n,
                                         None if "bitmaps" in null else buf.ctypes.data, None if "row_words" in null else words.ctypes.data, cnt.ctypes.data, None)
    msg = (e._L.acl_last_error() or b"").decode()
    assert (buf == 0xFFFFFFFF).all() and (cnt == 7).all()  # no GPU: nothing is ever written
    return rc, msg


def test_validation_comes_before_the_engines_mode(eng):
    import aclgpu
    e = eng
    doc, grp = e.type_id("doc"), e.type_id("group")
    view, member = e.relation_id("doc", "view"), e.relation_id("group", "member")
    assert e.object_count("doc") == 40
    good, words = [(doc, view), (grp, member)], [2, 1]
    # nothing asked: ACL_OK, whatever the engine's mode and the pointers
    assert raw_call(e, [], [], n=1)[0] == 0 and raw_call(e, good, words, n=0)[0] == 0
    assert raw_call(e, good, words, n=0, null=("targets", "sids", "bitmaps", "row_words"))[0] == 0
    # a NULL pointer where one is needed
    for which in ("targets", "sids", "bitmaps", "row_words"):
        assert raw_call(e, good, words, null=(which,))[0] == aclgpu.ERR_INVALID_ARGUMENT, which
    # an unknown type or member: FAILED_PRECONDITION, the message names the target
    for bad in ([(doc, view), (99, 0)], [(doc, view), (grp, 5)], [(doc, view), (grp, -1)]):
        rc, msg = raw_call(e, bad, words)
        assert rc == aclgpu.ERR_FAILED_PRECONDITION and "target 1" in msg, (bad, msg)
    rc, msg = raw_call(e, [(-1, 0)] + good, [1] + words)
    assert rc == aclgpu.ERR_FAILED_PRECONDITION and "target 0" in msg
    assert raw_call(e, good, words, stype="group", srel=9)[0] == aclgpu.ERR_FAILED_PRECONDITION  # (the subject's relation)
    # ... before the rows' sizes are looked at
    rc, msg = raw_call(e, [(doc, view), (99, 0)], [0, 0])
    assert rc == aclgpu.ERR_FAILED_PRECONDITION
    # a row one word too narrow: INVALID_ARGUMENT, the message names the target
    rc, msg = raw_call(e, good, [1, 1])
    assert rc == aclgpu.ERR_INVALID_ARGUMENT and "target 0" in msg and "bitmap too small" in msg
    rc, msg = raw_call(e, good, [2, 0])
    assert rc == aclgpu.ERR_INVALID_ARGUMENT and "target 1" in msg
    # everything in order (duplicates and wide rows included): only now does the store-only engine say so
    for tg, ww in ((good, words), (good + good, words + [5, 9]), ([(doc, view)], [2])):
        rc, msg = raw_call(e, tg, ww, n=3)
        assert rc == aclgpu.ERR_UNAVAILABLE and "store-only" in msg, (tg, msg)


def test_access_review_validates_then_refuses_on_a_store_only_engine(eng):
    import aclgpu
    e = eng
    for args, code in ((("user", "", ""), aclgpu.ERR_INVALID_ARGUMENT), (("user", "bad id!", ""), aclgpu.ERR_INVALID_ARGUMENT), (("nosuch", "u", ""), aclgpu.ERR_FAILED_PRECONDITION),
                       (("group", "g", "nosuch"), aclgpu.ERR_FAILED_PRECONDITION), (("user", "u", ""), aclgpu.ERR_UNAVAILABLE), (("group", "g", "member"), aclgpu.ERR_UNAVAILABLE)):
        with pytest.raises(aclgpu.AclError) as ei:
            e.access_review(*args)
        assert ei.value.code == code, args
    from aclgpu._lib import ReviewRow, Target
    rows, n, bms = C.POINTER(ReviewRow)(), C.c_size_t(5), C.POINTER(C.c_uint32)()
    bad = (Target * 2)(Target(e.type_id("doc"), 0), Target(e.type_id("doc"), 17))
    rc = e._L.acl_access_review(e._h, b"user", b"u", b"", bad, 2, None, C.byref(rows), C.byref(n), C.byref(bms))
    assert rc == aclgpu.ERR_FAILED_PRECONDITION and "target 1" in e._L.acl_last_error().decode() and not rows and not bms and n.value == 0
    assert e._L.acl_access_review(e._h, b"user", b"u", b"", None, 0, None, None, C.byref(n), C.byref(bms)) == aclgpu.ERR_INVALID_ARGUMENT
    # ids -> names of the schema, the way the review's rows are spelled
    assert e.schema_name(e.type_id("doc")) == "doc" and e.schema_name(e.type_id("doc"), e.relation_id("doc", "view")) == "view"
    assert e.schema_name(99) is None and e.schema_name(e.type_id("doc"), 17) is None


class FakeLib:
    """stands in for the library: records the call's layout and fills every row with its (subject, target) number"""

    def __init__(self, counts):
        self.counts = counts

    def acl_type_id(self, _h, name):
        return {b"user": 0, b"group": 1, b"doc": 2}[name]

    def acl_relation_id(self, _h, t, name):
        return {b"member": 0, b"viewer": 0, b"owner": 1, b"view": 2}[name]

    def acl_object_count(self, _h, t):
        return self.counts[t]

    def acl_lookup_resources_multi(self, _h, tg, T, stype, srel, sids, n, bitmaps, row_words, counts, opts):
        self.seen = dict(T=T, stype=stype, srel=srel, n=n, targets=[(tg[j].rtype, tg[j].permission) for j in range(T)])
        ww = np.ctypeslib.as_array(C.cast(row_words, C.POINTER(C.c_size_t)), shape=(T,))
        self.seen["row_words"] = [int(x) for x in ww]
        stride = int(ww.sum())
        flat = np.ctypeslib.as_array(C.cast(bitmaps, C.POINTER(C.c_uint32)), shape=(n * max(1, stride),))
        cn = np.ctypeslib.as_array(C.cast(counts, C.POINTER(C.c_uint64)), shape=(n * T,))
        for i in range(n):
            off = 0
            for j in range(T):  # row of (subject i, target j): bitmaps + i * stride + off[j]
                flat[i * stride + off:i * stride + off + int(ww[j])] = 100 * i + j
                cn[i * T + j] = 1000 * i + j
                off += int(ww[j])
        return 0


def test_python_wrapper_lays_the_rows_out_as_the_header_says(aclgpu_lib):
    import aclgpu
    e = aclgpu.Engine.__new__(aclgpu.Engine)
    e._h = C.c_void_p(1)
    e._L = FakeLib({0: 10, 1: 33, 2: 100})  # group: 2 words, doc: 4 words
    try:
        targets = [("doc", "view"), ("group", "member"), ("doc", "owner")]
        rows, counts = e.lookup_ids_multi(targets, "group", "member", [5, 6, 7])
        seen = e._L.seen
        assert seen["targets"] == [(2, 2), (1, 0), (2, 1)] and seen["row_words"] == [4, 2, 4] and (seen["stype"], seen["srel"], seen["n"], seen["T"]) == (1, 0, 3, 3)
        assert [r.shape for r in rows] == [(3, 4), (3, 2), (3, 4)] and counts.shape == (3, 3) and counts.dtype == np.uint64 and all(r.dtype == np.uint32 for r in rows)
        for i in range(3):
            for j in range(3):
                assert (rows[j][i] == 100 * i + j).all() and counts[i, j] == 1000 * i + j
        rows, counts = e.lookup_ids_multi([("doc", "view")], "user", "", [1])
        assert e._L.seen["srel"] == -1 and rows[0].shape == (1, 4) and counts.shape == (1, 1)
    finally:
        e._h = None  # (nothing to close)


def test_stats_end_in_the_two_new_fields(aclgpu_lib):
    from aclgpu._lib import Stats
    assert [n for n, _t in Stats._fields_][-2:] == ["rev_multi_passes", "rev_multi_ms"]
    assert Stats._fields_[-2][1] is C.c_uint64 and Stats._fields_[-1][1] is C.c_double

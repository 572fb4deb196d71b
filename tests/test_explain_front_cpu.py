"""The refusals of the six Explain entry points (acl_explain*, acl_explain_proof*, acl_explain_denial*) that are decided before an evaluation begins:
their return codes, their acl_last_error texts and the order in which they are tested, held to tests/golden/explain_front_refusals.json.  The fixture was
recorded before the three forms were given one call front (`python -m tests.test_explain_front_cpu --record` writes it); no case needs a GPU."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "explain_front_refusals.json")

BAN = """
definition user {}
definition doc {
  relation viewer: user
  relation banned: user
  permission view = viewer - banned
}
"""
FORMS = ("explain", "explain_proof", "explain_denial")
BULK_OUTPUTS = {"explain": ("hop_off", "hops"), "explain_proof": ("hop_off", "hops", "absent_off", "absent"), "explain_denial": ("grant_off", "grants")}
ONE_ARGS = ("item", "perm_out", "err_out", "text_out")


def _outcome(m, call):
    """[code, acl_last_error text] of a refused call; [0, ""] of one that returns"""
    try:
        call()
    except m.AclError as x:
        return [x.code, x.message]
    return [0, ""]


def _raw_bulk(m, e, form, n, null):
    """the raw bulk symbol with one argument NULL (`null`: "items" or one of the form's outputs)"""
    items = np.zeros(max(n, 1), dtype=m.ITEM_DTYPE)
    perm, err, flags = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.uint8)
    off, off2 = np.zeros(n + 1, dtype=np.uint32), np.zeros(n + 1, dtype=np.uint32)
    fn = getattr(e._L, "acl_" + form + "_bulk_ids")
    recs = C.POINTER(m._lib.Grant if form == "explain_denial" else m._lib.ExplainHop)()
    recs2 = C.c_void_p()
    outs = [off.ctypes.data, C.byref(recs)] + ([off2.ctypes.data, C.byref(recs2)] if form == "explain_proof" else [])
    if null != "items":
        outs[BULK_OUTPUTS[form].index(null)] = None
    rc = fn(e._h, None if null == "items" else items.ctypes.data, n, perm.ctypes.data, err.ctypes.data, flags.ctypes.data, *outs, None)
    e._check(rc)
    e._L.acl_free(recs)
    e._L.acl_free(recs2)


def _raw_one(m, e, form, null):
    """the raw one-item symbol with one argument NULL"""
    it = m._lib.CheckItem(b"doc", b"d", b"view", b"user", b"a", b"")
    p, x, f, txt = C.c_uint8(), C.c_int32(), C.c_uint32(), C.c_void_p()
    args = dict(item=C.byref(it), perm_out=C.byref(p), err_out=C.byref(x), text_out=C.byref(txt))
    args[null] = None
    rc = getattr(e._L, "acl_" + form)(e._h, args["item"], args["perm_out"], args["err_out"], C.byref(f), args["text_out"], None)
    e._check(rc)
    e._L.acl_free(txt)


def collect(m):
    got = {}
    with m.Engine(BAN, store_only=True) as e, m.Engine(BAN, store_only=True, per_item_validation=True) as lenient, m.Engine(store_only=True) as bare:
        e.touch(("doc", "d", "viewer", "user", "a", ""))
        lenient.touch(("doc", "d", "viewer", "user", "a", ""))
        items = e.make_items("doc", "view", [e.find("doc", "d")], "user", "", [e.find("user", "a")])
        for form in FORMS:
            bulk, one = getattr(e, form + "_ids"), getattr(e, form)
            got[form + "_ids/store_only/n=1"] = _outcome(m, lambda: bulk(items))
            got[form + "_ids/store_only/n=0"] = _outcome(m, lambda: bulk(items[:0]))
            for out in BULK_OUTPUTS[form]:
                got[form + "_ids/null/" + out] = _outcome(m, lambda: _raw_bulk(m, e, form, 1, out))
                got[form + "_ids/null/" + out + "/n=0"] = _outcome(m, lambda: _raw_bulk(m, e, form, 0, out))
            got[form + "_ids/null/items"] = _outcome(m, lambda: _raw_bulk(m, e, form, 1, "items"))
            for arg in ONE_ARGS:
                got[form + "/null/" + arg] = _outcome(m, lambda: _raw_one(m, e, form, arg))
            got[form + "/no_schema"] = _outcome(m, lambda: getattr(bare, form)("doc", "d", "view", "user", "a"))
            got[form + "/store_only"] = _outcome(m, lambda: one("doc", "d", "view", "user", "a"))
            got[form + "/bad_id"] = _outcome(m, lambda: one("doc", "not an id", "view", "user", "a"))
            got[form + "/bad_id/per_item_validation"] = _outcome(m, lambda: getattr(lenient, form)("doc", "not an id", "view", "user", "a"))
            got[form + "/unknown_type"] = _outcome(m, lambda: one("nothing", "d", "view", "user", "a"))
            got[form + "/unknown_type/per_item_validation"] = _outcome(m, lambda: getattr(lenient, form)("nothing", "d", "view", "user", "a"))
    return got


@pytest.fixture(scope="module")
def aclgpu(aclgpu_lib):
    import aclgpu as m
    return m


@pytest.fixture(scope="module")
def got(aclgpu):
    return collect(aclgpu)


@pytest.fixture(scope="module")
def want():
    with open(FIXTURE) as f:
        return json.load(f)


def test_every_refusal_is_the_recorded_one(got, want):
    assert sorted(got) == sorted(want)
    for case in sorted(want):
        print(case, got[case])
        assert got[case] == want[case], case


def test_the_api_validation_comes_before_the_store_only_refusal(aclgpu, got):
    for form in FORMS:
        assert got[form + "/bad_id"][0] == aclgpu.ERR_INVALID_ARGUMENT, form
        assert got[form + "/store_only"][0] == aclgpu.ERR_UNAVAILABLE, form


def test_the_forms_agree_where_the_recorded_ones_do(got, want):
    """whatever the recorded library answers alike for two entry points, this one answers alike too (the store-only text of all six, for one)"""
    def suffixes(form):
        return {case[len(form):] for case in want if case.startswith(form + "/") or case.startswith(form + "_ids/")}
    checked = 0
    for a in FORMS:
        for b in FORMS:
            for s in sorted(suffixes(a) & suffixes(b)):
                if a < b and want[a + s] == want[b + s]:
                    assert got[a + s] == got[b + s], (a, b, s)
                    checked += 1
    assert checked
    store_only = {tuple(got[form + s]) for form in FORMS for s in ("_ids/store_only/n=1", "_ids/store_only/n=0", "/store_only")}
    assert len(store_only) == 1 and next(iter(store_only))[1].endswith("Explain is unavailable")


if __name__ == "__main__" and "--record" in sys.argv:
    sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "spicedb-kubeapi-proxy_amd")]
    import aclgpu as _m
    with open(FIXTURE, "w") as _f:
        json.dump(collect(_m), _f, indent=1, sort_keys=True)
        _f.write("\n")

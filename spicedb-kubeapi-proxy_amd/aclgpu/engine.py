"""Engine: thin Python handle over the C ABI (include/aclgpu.h).

Numeric entry points take / return numpy arrays; the string entry points mirror
the request shapes the reference builds in pkg/authz/check.go:23-39 and
pkg/authz/lookups.go:49-62.
"""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np

from . import _lib
from ._lib import CallOpts, CheckItem, Completion, Config, ExplainHop, ExplainOpRec, Filter, Grant, READ_CB, Relationship, Stats, Update, WATCH_CB, WATCH_CHECK_CB, WatchChange

PERM_UNSPECIFIED, PERM_NO, PERM_HAS, PERM_CONDITIONAL = 0, 1, 2, 3
OP_CREATE, OP_TOUCH, OP_DELETE = 1, 2, 3
PRE_MUST_NOT_MATCH, PRE_MUST_MATCH = 1, 2
ERR_INVALID_ARGUMENT, ERR_NOT_FOUND, ERR_ALREADY_EXISTS, ERR_RESOURCE_EXHAUSTED, ERR_FAILED_PRECONDITION = 3, 5, 6, 8, 9
ERR_INTERNAL, ERR_UNAVAILABLE, ERR_DEPTH = 13, 14, 100
ERR_OUT_OF_RANGE = 11
ERR_CANCELLED, ERR_DEADLINE_EXCEEDED = 1, 4
WATCH_FROM_NOW = 0xFFFFFFFFFFFFFFFF
NO_RELATION = 0xFFFF

ITEM_DTYPE = np.dtype([("resource_type", "<u2"), ("permission", "<u2"), ("resource_id", "<u4"), ("subject_type", "<u2"),
                       ("subject_relation", "<u2"), ("subject_id", "<u4")])
assert ITEM_DTYPE.itemsize == 16
WATCHER_FROM_NOW = 1  # ACL_WATCHER_FROM_NOW
PAGE_FROM_START = 0xFFFFFFFF  # ACL_PAGE_FROM_START: a page's after_id "before id 0"
SUBJECT_REF_DTYPE = np.dtype([("stype", "<i4"), ("srel", "<i4"), ("id", "<u4"), ("reserved", "<u4")])  # acl_subject_ref_t
DERIVE_ANY_REVISION = 1  # ACL_DERIVE_ANY_REVISION: the sources of a derived cursor may have been opened at different revisions
WATCH_CHANGE_WILDCARD = 1  # ACL_WATCH_CHANGE_WILDCARD (a record's `reserved`, subject-direction sets)
WATCH_CHANGE_DTYPE = np.dtype([("watcher", "<u4"), ("resource_id", "<u4"), ("gained", "<u4"), ("reserved", "<u4")])  # acl_watch_change_t
assert WATCH_CHANGE_DTYPE.itemsize == C.sizeof(WatchChange) == 16
HOP_DTYPE = np.dtype([("rtype", "<u2"), ("relation", "<u2"), ("rid", "<u4"), ("stype", "<u2"), ("srel", "<u2"), ("sid", "<u4"), ("flags", "<u4")])  # acl_explain_hop_t
assert HOP_DTYPE.itemsize == C.sizeof(ExplainHop) == 20
EXPLAIN_OP_DTYPE = np.dtype([("rtype", "<u2"), ("relation", "<u2"), ("stype", "<u2"), ("srel", "<u2"), ("slot", "<u4"), ("dlevel", "<u4"), ("kind", "<u4")])  # acl_explain_op_t
assert EXPLAIN_OP_DTYPE.itemsize == C.sizeof(ExplainOpRec) == 20
GRANT_DTYPE = np.dtype([("rtype", "<u2"), ("relation", "<u2"), ("rid", "<u4"), ("level", "<u4")])  # acl_grant_t
assert GRANT_DTYPE.itemsize == C.sizeof(Grant) == 12
EXPLAIN_DENIAL = 8                              # ACL_EXPLAIN_DENIAL: the item's grants are ALL single relationships whose write grants it
EXPLAIN_REVOKE = 16                             # ACL_EXPLAIN_REVOKE: the item's cuts are ALL single relationships whose delete revokes it
HOP_WILDCARD = 1                                # ACL_HOP_WILDCARD
EXPLAIN_WITNESS, EXPLAIN_UNSUPPORTED = 1, 2     # per-item flags of Explain
HOP_SEGMENT = 2                                 # ACL_HOP_SEGMENT: the hop starts a new chain of a proof
EXPLAIN_PROOF = 4                               # ACL_EXPLAIN_PROOF: hops + absences prove the item
PROOF_MAX_RECORDS = 65536                       # ACL_PROOF_MAX_RECORDS


class AclError(Exception):
    """Carries the gRPC status code the Go shim would return (status.Code(err))."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"[{code}] {msg}")
        self.code = code
        self.message = msg


def _b(s):
    return None if s is None else s.encode()


class Engine:
    names_invalid_fields = True  # a request the API's validation refuses fails with a message naming the item, the field, the value and the pattern (tests/kat_runner.py)

    def __init__(self, schema: str | None = None, relationships: str | None = None, device: int = -1, frontier_entries: int = 0,
                 max_sub_batch: int = 0, store_only: bool = False, contexts: int = 0, devices=None, per_item_validation: bool = False,
                 lenient_lookup: bool = False, eager_contexts: bool = False):
        """devices: HIP ordinals of the replicas (acl_open_replicas: ONE store and one set of name tables in front of one HBM snapshot per
        entry; a device may be listed more than once); default one replica on `device`."""
        self._L = _lib.load()
        cfg = Config(device, frontier_entries, max_sub_batch, (1 if store_only else 0) | (2 if per_item_validation else 0) | (4 if lenient_lookup else 0) | (8 if eager_contexts else 0), contexts, 0)
        # (ACL_FLAG_STORE_ONLY | _PER_ITEM_VALIDATION | _LENIENT_LOOKUP | _EAGER_CONTEXTS)
        h = C.c_void_p()
        if devices:
            arr = (C.c_int32 * len(devices))(*[int(d) for d in devices])
            rc = self._L.acl_open_replicas(C.byref(cfg), arr, len(devices), C.byref(h))
        else:
            rc = self._L.acl_open(C.byref(cfg), C.byref(h))
        self._h = h if rc == 0 else None
        self._check(rc)
        if schema is not None:
            self.load_bootstrap(schema, relationships)

    # ---- plumbing
    def _check(self, rc):
        if rc:
            raise AclError(rc, (self._L.acl_last_error() or b"").decode())

    def close(self):
        if getattr(self, "_h", None):
            self._L.acl_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def load_bootstrap(self, schema: str, relationships: str | None = None):
        s = schema.encode()
        r = relationships.encode() if relationships else None
        self._check(self._L.acl_load_bootstrap(self._h, s, len(s), r, len(r) if r else 0))

    def load_bootstrap_yaml(self, yaml_text):
        """The bootstrap FILE form (pkg/spicedb/bootstrap.yaml; spicedb.go:19-24): YAML `{schema, relationships}` documents."""
        y = yaml_text if isinstance(yaml_text, bytes) else yaml_text.encode()
        self._check(self._L.acl_load_bootstrap_yaml(self._h, y, len(y)))

    # ---- ids
    def type_id(self, t: str) -> int:
        return self._L.acl_type_id(self._h, _b(t))

    def relation_id(self, t: str, r: str | None) -> int:
        return -1 if not r else self._L.acl_relation_id(self._h, self.type_id(t), _b(r))

    def schema_name(self, type_id: int, member: int = -1):
        """acl_schema_name_copy: the name of definition `type_id`, or of its relation / permission `member`; None when there is none."""
        buf = C.create_string_buffer(256)
        n = self._L.acl_schema_name_copy(self._h, int(type_id), int(member), buf, len(buf))
        return None if n < 0 else buf.value.decode()

    def intern(self, t: str, oid: str) -> int:
        out = C.c_uint32()
        self._check(self._L.acl_intern(self._h, self.type_id(t), _b(oid), C.byref(out)))
        return out.value

    def find(self, t: str, oid: str):
        out = C.c_uint32()
        rc = self._L.acl_find(self._h, self.type_id(t), _b(oid), C.byref(out))
        return out.value if rc == 0 else None

    def object_name(self, t: str, i: int):
        """acl_object_name_copy: the name is copied out under the names lock (an id that takes part in no relationship may be renamed later)"""
        buf = C.create_string_buffer(256)
        while True:  # (the id may be given a longer name between two copies: a length is only used once it fits the buffer it was copied into)
            n = self._L.acl_object_name_copy(self._h, self.type_id(t), int(i), buf, len(buf))
            if n < 0:
                return None
            if n < len(buf):
                return buf.raw[:n].decode()
            buf = C.create_string_buffer(n + 1)

    def object_count(self, t: str) -> int:
        return self._L.acl_object_count(self._h, self.type_id(t))

    # ---- writes
    @staticmethod
    def _mkrel(r, expires=0):
        rt, rid, rel, st, sid, srel = r
        return Relationship(_b(rt), _b(rid), _b(rel), _b(st), _b(sid), _b(srel or ""), int(expires))

    @staticmethod
    def _mkfilter(op=0, rtype=None, rid=None, rel=None, stype=None, sid=None, srel=None):
        return Filter(op, _b(rtype), _b(rid), _b(rel), _b(stype), _b(sid), _b(srel))

    def write(self, updates, preconditions=()):
        """updates: [(op, (rt, rid, rel, st, sid, srel) | 'text', expires?)]; preconditions: [(op, {filter kwargs})]."""
        from .text import parse_relationship
        ups = (Update * max(1, len(updates)))()
        for i, u in enumerate(updates):
            r = parse_relationship(u[1]) if isinstance(u[1], str) else u[1]
            ups[i] = Update(u[0], self._mkrel(r, u[2] if len(u) > 2 else 0))
        pre = (Filter * max(1, len(preconditions)))()
        for i, (op, f) in enumerate(preconditions):
            pre[i] = self._mkfilter(op, **f)
        rev = C.c_uint64()
        self._check(self._L.acl_write(self._h, ups, len(updates), pre, len(preconditions), C.byref(rev)))
        return rev.value

    def touch(self, *rels):
        return self.write([(OP_TOUCH, r) for r in rels])

    def delete_by_filter(self, preconditions=(), **f):
        """DeleteRelationships; preconditions [(op, {filter kwargs})] are evaluated against the pre-delete state."""
        n, rev = C.c_uint64(), C.c_uint64()
        flt = self._mkfilter(0, **f)
        pre = (Filter * max(1, len(preconditions)))()
        for i, (op, pf) in enumerate(preconditions):
            pre[i] = self._mkfilter(op, **pf)
        self._check(self._L.acl_delete_by_filter_pre(self._h, C.byref(flt), pre, len(preconditions), C.byref(n), C.byref(rev)))
        return n.value

    def read(self, **f):
        out = []

        def cb(_u, rp):
            r = rp.contents
            out.append((r.resource_type.decode(), r.resource_id.decode(), r.relation.decode(), r.subject_type.decode(), r.subject_id.decode(),
                        (r.subject_relation or b"").decode(), r.expires_at))

        flt = self._mkfilter(0, **f)
        self._check(self._L.acl_read(self._h, C.byref(flt), READ_CB(cb), None))
        return out

    def add_edges(self, rtype, rel, stype, srel, res, subj):
        res = np.ascontiguousarray(res, dtype=np.uint32)
        subj = np.ascontiguousarray(subj, dtype=np.uint32)
        assert res.shape == subj.shape
        # srel "*": `stype:*` relationships, one per entry of res (subj is ignored)
        self._check(self._L.acl_add_edges(self._h, self.type_id(rtype), self.relation_id(rtype, rel), self.type_id(stype),
                                          -2 if srel == "*" else self.relation_id(stype, srel), res.size, res.ctypes.data, subj.ctypes.data))

    def set_now(self, t: int):
        self._check(self._L.acl_set_now(self._h, int(t)))

    @property
    def revision(self):
        return self._L.acl_revision(self._h)

    def snapshot(self):
        self._check(self._L.acl_snapshot(self._h))

    # ---- checks
    def check_bulk(self, items):
        """items: [(rt, rid, perm, st, sid, srel)] -> (perms list, errs list); index aligned (check.go:54-57)."""
        n = len(items)
        arr = (CheckItem * max(1, n))()
        for i, it in enumerate(items):
            arr[i] = CheckItem(*[_b(x if x is not None else "") for x in it])
        perm = np.zeros(max(1, n), dtype=np.uint8)
        err = np.zeros(max(1, n), dtype=np.int32)
        self._check(self._L.acl_check_bulk(self._h, arr, n, perm.ctypes.data, err.ctypes.data))
        return perm[:n].tolist(), err[:n].tolist()

    def check(self, rt, rid, perm, st, sid, srel=""):
        """CheckPermission: (permissionship, error code).  A request the API's validation refuses fails as a whole (validate.hpp): for a
        single check the call's InvalidArgument is the item's."""
        try:
            p, e = self.check_bulk([(rt, rid, perm, st, sid, srel)])
        except AclError as x:
            if x.code == ERR_INVALID_ARGUMENT:
                return 0, x.code
            raise
        return p[0], e[0]

    def make_items(self, rtype, perm, res, stype, srel, subj):
        """Interned 16-byte items (acl_item_t) for one (type#perm, subject class) and id arrays."""
        res = np.asarray(res, dtype=np.uint32)
        items = np.zeros(res.size, dtype=ITEM_DTYPE)
        items["resource_type"] = self.type_id(rtype)
        items["permission"] = self.relation_id(rtype, perm)
        items["resource_id"] = res
        items["subject_type"] = self.type_id(stype)
        r = self.relation_id(stype, srel)
        items["subject_relation"] = NO_RELATION if r < 0 else r
        items["subject_id"] = np.asarray(subj, dtype=np.uint32)
        return items

    def check_bulk_ids(self, items: np.ndarray):
        items = np.ascontiguousarray(items, dtype=ITEM_DTYPE)
        n = items.size
        perm = np.zeros(max(1, n), dtype=np.uint8)
        err = np.zeros(max(1, n), dtype=np.int32)
        self._check(self._L.acl_check_bulk_ids(self._h, items.ctypes.data, n, perm.ctypes.data, err.ctypes.data))
        return perm[:n], err[:n]

    def check_bulk_ids_into(self, items: np.ndarray, perm: np.ndarray, err: np.ndarray):
        """acl_check_bulk_ids into caller-owned arrays (e.g. views of host_alloc memory: no staging copy)."""
        self._check(self._L.acl_check_bulk_ids(self._h, items.ctypes.data, items.size, perm.ctypes.data, err.ctypes.data))

    def make_check_strings(self, rtype, perm, res, stype, subj, srel=""):
        """A prepared acl_check_item_t array whose object ids are the DECIMAL numeric ids (bench.py's string leg)."""
        n = len(res)
        arr = (CheckItem * max(1, n))()
        rt, pm, st, sr = _b(rtype), _b(perm), _b(stype), _b(srel)
        keep = []
        for i in range(n):
            a, b = str(int(res[i])).encode(), str(int(subj[i])).encode()
            keep.append(a)
            keep.append(b)
            arr[i] = CheckItem(rt, a, pm, st, b, sr)
        return arr, n, keep

    def make_check_strings_named(self, items):
        """A prepared acl_check_item_t array of [(rt, rid, perm, st, sid, srel)] (the ctypes marshalling done once, outside any timing)."""
        n = len(items)
        arr = (CheckItem * max(1, n))()
        keep = []
        for i, it in enumerate(items):
            bs = [_b(x if x is not None else "") for x in it]
            keep.append(bs)
            arr[i] = CheckItem(*bs)
        return arr, n, keep

    def make_check_views(self, items):
        """A prepared acl_check_item_v_t array ({pointer, length} x 6 per item) of [(rt, rid, perm, st, sid, srel)]: every distinct string is
        stored once in one blob WITHOUT a NUL behind it, and equal strings share their bytes -- as a cgo shim pointing at Go strings would."""
        n = len(items)
        blob = bytearray()
        where = {}
        views = np.zeros((max(1, n), 6, 2), dtype=np.uint64)
        offs = np.zeros((max(1, n), 6), dtype=np.int64)
        for i, it in enumerate(items):
            for f, x in enumerate(it):
                b = _b(x if x is not None else "") or b""
                if f == 5 and not b:
                    offs[i, f] = -1  # an absent subject relation is {NULL, 0}
                    continue
                at = where.get(b)
                if at is None:
                    at = where[b] = len(blob)
                    blob += b
                offs[i, f] = at
                views[i, f, 1] = len(b)
        buf = np.frombuffer(bytes(blob) or b"\0", dtype=np.uint8).copy()
        views[:, :, 0] = np.where(offs >= 0, buf.ctypes.data + offs, 0).astype(np.uint64)
        return views, n, buf

    def check_bulk_views(self, prepared, cancel=None, timeout_s=None):
        """acl_check_bulk_v; with `cancel` (a ctypes c_int32 the caller raises) or `timeout_s`: acl_check_bulk_v_opts -- CheckBulkPermissions(ctx, ...)"""
        views, n, _blob = prepared
        perm = np.zeros(max(1, n), dtype=np.uint8)
        err = np.zeros(max(1, n), dtype=np.int32)
        if cancel is None and timeout_s is None:
            self._check(self._L.acl_check_bulk_v(self._h, views.ctypes.data, n, perm.ctypes.data, err.ctypes.data))
        else:
            o = _lib.CallOpts(C.pointer(cancel) if cancel is not None else None, int((timeout_s or 0) * 1e9))
            self._check(self._L.acl_check_bulk_v_opts(self._h, views.ctypes.data, n, perm.ctypes.data, err.ctypes.data, C.byref(o)))
        return perm[:n], err[:n]

    def resolve_bulk_views(self, prepared):
        """acl_resolve_bulk_v: the prepared views as the 16-byte items of the id entry points (no device pass) + a per-item error array."""
        views, n, _blob = prepared
        items = np.zeros(max(1, n), dtype=ITEM_DTYPE)
        err = np.zeros(max(1, n), dtype=np.int32)
        self._check(self._L.acl_resolve_bulk_v(self._h, views.ctypes.data, n, items.ctypes.data, err.ctypes.data))
        return items[:n], err[:n]

    def check_bulk_prepared(self, prepared):
        arr, n, _keep = prepared
        perm = np.zeros(max(1, n), dtype=np.uint8)
        err = np.zeros(max(1, n), dtype=np.int32)
        self._check(self._L.acl_check_bulk(self._h, arr, n, perm.ctypes.data, err.ctypes.data))
        return perm[:n], err[:n]

    @staticmethod
    def _opts(cancel=None, timeout_s=None):
        """cancel: a ctypes.c_int32 the caller sets non-zero to abandon the call (the C side of ctx.Done())."""
        if cancel is None and not timeout_s:
            return None
        return CallOpts(C.pointer(cancel) if cancel is not None else None, int((timeout_s or 0) * 1e9))

    def check_bulk_ids_opts(self, items: np.ndarray, cancel=None, timeout_s=None):
        items = np.ascontiguousarray(items, dtype=ITEM_DTYPE)
        n = items.size
        perm = np.zeros(max(1, n), dtype=np.uint8)
        err = np.zeros(max(1, n), dtype=np.int32)
        o = self._opts(cancel, timeout_s)
        self._check(self._L.acl_check_bulk_ids_opts(self._h, items.ctypes.data, n, perm.ctypes.data, err.ctypes.data, C.byref(o) if o else None))
        return perm[:n], err[:n]

    # ---- pipelined host-buffer path: pinned request / answer arrays + submit / wait
    def host_alloc(self, nbytes: int) -> np.ndarray:
        """Page-locked host memory as a uint8 array (free with host_free): DMA'd directly by check_bulk_ids / submit."""
        p = C.c_void_p()
        self._check(self._L.acl_host_alloc(self._h, int(nbytes), C.byref(p)))
        buf = (C.c_uint8 * int(nbytes)).from_address(p.value)
        a = np.frombuffer(buf, dtype=np.uint8)
        a.flags.writeable = True
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[a.ctypes.data] = p.value
        return a

    def host_free(self, a: np.ndarray):
        p = getattr(self, "_pinned", {}).pop(a.ctypes.data, None)
        if p is not None and self._h:
            self._check(self._L.acl_host_free(self._h, p))

    def submit_ids(self, items: np.ndarray, perm: np.ndarray, err: np.ndarray):
        """acl_check_bulk_ids_submit: returns a ticket; the arrays must stay alive (and untouched) until wait()."""
        t = C.c_void_p()
        self._check(self._L.acl_check_bulk_ids_submit(self._h, items.ctypes.data, items.size, perm.ctypes.data, err.ctypes.data, C.byref(t)))
        return t

    def wait(self, ticket):
        self._check(self._L.acl_ticket_wait(self._h, ticket))

    def check_bulk_ids_device(self, d_items: int, n: int, d_perm: int, d_err: int = 0):
        """Device pointers (ints); asynchronous after return only w.r.t. the output buffers' readers on acl_stream."""
        self._check(self._L.acl_check_bulk_ids_device(self._h, d_items, n, d_perm, d_err or None))

    def sync(self):
        self._check(self._L.acl_sync(self._h))

    @property
    def stream(self) -> int:
        return self._L.acl_stream(self._h) or 0

    # ---- callers either side of the kernels
    def check_bulk_keep(self, items, item_off):
        """filterItemsWithBulkPermissions (postfilter.go:58-182): items = all resolved pairs [(rt, rid, perm, st, sid, srel)],
        pairs [item_off[i], item_off[i+1]) belong to list item i -> keep mask (uint8[K])."""
        n = len(items)
        arr = (CheckItem * max(1, n))()
        for i, it in enumerate(items):
            arr[i] = CheckItem(*[_b(x if x is not None else "") for x in it])
        off = np.ascontiguousarray(item_off, dtype=np.uint32)
        keep = np.zeros(max(1, off.size - 1), dtype=np.uint8)
        self._check(self._L.acl_check_bulk_keep(self._h, arr, n, off.ctypes.data, off.size - 1, keep.ctypes.data))
        return keep[:off.size - 1]

    def check_bulk_keep_views(self, prepared, item_off):
        """acl_check_bulk_keep_v: the pairs as {pointer, length} views (make_check_views); a call whose pairs share type, permission and subject is
        answered by one reverse walk + bit tests (stats()["keep_route_calls"])."""
        views, n, _blob = prepared
        off = np.ascontiguousarray(item_off, dtype=np.uint32)
        keep = np.zeros(max(1, off.size - 1), dtype=np.uint8)
        self._check(self._L.acl_check_bulk_keep_v(self._h, views.ctypes.data, n, off.ctypes.data, off.size - 1, keep.ctypes.data))
        return keep[:off.size - 1]

    @staticmethod
    def make_check_packed(items):
        """An acl_packed_request_t of [(rt, rid, perm, st, sid, srel)]: every distinct string once in a dictionary, six u32 indices per item (an absent
        subject relation: ACL_PACKED_NONE) -- what the cgo shim fills while it walks a kube list.  -> (request struct, the arrays it points into)"""
        n = len(items)
        where, blob, offsets = {}, bytearray(), [0]
        idx = np.full((max(1, n), 6), 0xFFFFFFFF, dtype=np.uint32)
        for i, it in enumerate(items):
            for f, x in enumerate(it):
                b = _b(x if x is not None else "") or b""
                if f == 5 and not b:
                    continue
                k = where.get(b)
                if k is None:
                    k = where[b] = len(offsets) - 1
                    blob += b
                    offsets.append(len(blob))
                idx[i, f] = k
        buf = np.frombuffer(bytes(blob) or b"\0", dtype=np.uint8).copy()
        offs = np.asarray(offsets, dtype=np.uint32)
        rq = _lib.PackedRequest(buf.ctypes.data, offs.ctypes.data, len(offsets) - 1, 0, idx.ctypes.data, n)
        return rq, (buf, offs, idx)

    def check_bulk_packed(self, prepared):
        rq, _keep_alive = prepared
        n = rq.n_items
        perm = np.zeros(max(1, n), dtype=np.uint8)
        err = np.zeros(max(1, n), dtype=np.int32)
        self._check(self._L.acl_check_bulk_packed(self._h, C.byref(rq), perm.ctypes.data, err.ctypes.data, None))
        return perm[:n], err[:n]

    def check_bulk_keep_packed(self, prepared, item_off):
        rq, _keep_alive = prepared
        off = np.ascontiguousarray(item_off, dtype=np.uint32)
        keep = np.zeros(max(1, off.size - 1), dtype=np.uint8)
        self._check(self._L.acl_check_bulk_keep_packed(self._h, C.byref(rq), off.ctypes.data, off.size - 1, keep.ctypes.data))
        return keep[:off.size - 1]

    def check_bulk_keep_ids(self, items: np.ndarray, item_off):
        items = np.ascontiguousarray(items, dtype=ITEM_DTYPE)
        off = np.ascontiguousarray(item_off, dtype=np.uint32)
        keep = np.zeros(max(1, off.size - 1), dtype=np.uint8)
        self._check(self._L.acl_check_bulk_keep_ids(self._h, items.ctypes.data, items.size, off.ctypes.data, off.size - 1, keep.ctypes.data))
        return keep[:off.size - 1]

    def check_bulk_keep_ids_device(self, d_items: int, n: int, d_item_off: int, k_items: int, d_keep: int):
        self._check(self._L.acl_check_bulk_keep_ids_device(self._h, d_items, n, d_item_off, k_items, d_keep))

    def filter_list_response(self, body: bytes, templates, user_name: str, request=None):
        """filterListResponse (postfilter.go:17-55) on the list response's bytes -> (filtered body, kept, total).
        request = (name, namespace, resource) of the kube request (rules.NewResolveInput's fallbacks, rules.go:315-342), or None."""
        from ._lib import ListRequest
        arr = (C.c_char_p * max(1, len(templates)))(*[_b(t) for t in templates])
        out, n, kept, total = C.c_void_p(), C.c_size_t(), C.c_uint64(), C.c_uint64()
        if request is not None:
            rq = ListRequest(_b(request[0] or ""), _b(request[1] or ""), _b(request[2] or ""))
            self._check(self._L.acl_filter_list_response_req(self._h, body, len(body), arr, len(templates), _b(user_name), C.byref(rq), C.byref(out), C.byref(n),
                                                             C.byref(kept), C.byref(total)))
        else:
            self._check(self._L.acl_filter_list_response(self._h, body, len(body), arr, len(templates), _b(user_name), C.byref(out), C.byref(n),
                                                         C.byref(kept), C.byref(total)))
        try:
            return C.string_at(out, n.value), kept.value, total.value
        finally:
            self._L.acl_free(out)

    BODY_LIST, BODY_TABLE, BODY_OBJECT = 0, 1, 2

    def prefilter_response(self, rtype: str, bitmap: np.ndarray, id_template: str, kind: int, body: bytes):
        """filterList / filterTable / filterObject (responsefilterer.go:349-416) on the kube response's bytes, with the LookupResources bitmap
        as the allowed set -> (filtered body, kept, total).  A single object outside the set raises AclError(code 7, "unauthorized")."""
        bm = np.ascontiguousarray(bitmap, dtype=np.uint32)
        out, n, kept, total = C.c_void_p(), C.c_size_t(), C.c_uint64(), C.c_uint64()
        self._check(self._L.acl_prefilter_response(self._h, self.type_id(rtype), bm.ctypes.data, bm.size, _b(id_template), kind, body, len(body), C.byref(out), C.byref(n),
                                                   C.byref(kept), C.byref(total)))
        try:
            return C.string_at(out, n.value), kept.value, total.value
        finally:
            self._L.acl_free(out)

    def bitmap_names(self, rtype: str, bitmap: np.ndarray, block: int = 512, buf_bytes: int = 1 << 16):
        """acl_bitmap_names: the names of a LookupResources bitmap's objects in id order, fetched a block per call (what the shim's stream does)."""
        bm = np.ascontiguousarray(bitmap, dtype=np.uint32)
        buf = C.create_string_buffer(buf_bytes)
        ends = np.zeros(block, dtype=np.uint32)
        cur, n = C.c_uint64(0), C.c_size_t()
        out = []
        while True:
            self._check(self._L.acl_bitmap_names(self._h, self.type_id(rtype), bm.ctypes.data, bm.size, C.byref(cur), buf, buf_bytes, ends.ctypes.data, block, C.byref(n)))
            if not n.value:
                return out
            raw, prev = buf.raw, 0
            for k in range(n.value):
                out.append(raw[prev:int(ends[k])].decode())
                prev = int(ends[k])

    def bitmap_test_names(self, rtype: str, bitmap: np.ndarray, object_ids):
        """prefilterResult.IsAllowed (lookups.go:25-36) over a LookupResources bitmap -> bool array."""
        bm = np.ascontiguousarray(bitmap, dtype=np.uint32)
        n = len(object_ids)
        arr = (C.c_char_p * max(1, n))(*[_b(x) for x in object_ids])
        out = np.zeros(max(1, n), dtype=np.uint8)
        self._check(self._L.acl_bitmap_test_names(self._h, self.type_id(rtype), bm.ctypes.data, bm.size, arr, n, out.ctypes.data))
        return out[:n].astype(bool)

    def watch_poll(self, after_revision: int, types=()):
        """-> (updates [(revision, op, (rt, rid, rel, st, sid, srel))], next cursor).  after_revision=WATCH_FROM_NOW: just the cursor."""
        out = []

        def cb(_u, rev, op, rp):
            r = rp.contents
            out.append((rev, op, (r.resource_type.decode(), r.resource_id.decode(), r.relation.decode(), r.subject_type.decode(),
                                  r.subject_id.decode(), (r.subject_relation or b"").decode())))

        tids = [self.type_id(t) for t in types]
        if any(t < 0 for t in tids):
            raise AclError(ERR_FAILED_PRECONDITION, "unknown object type in watch request")
        arr = (C.c_int * max(1, len(tids)))(*tids)
        cur = C.c_uint64()
        self._check(self._L.acl_watch_poll(self._h, after_revision, arr, len(tids), WATCH_CB(cb), None, C.byref(cur)))
        return out, cur.value

    def watch_wait(self, after_revision: int, types=(), timeout_s=None, cancel=None) -> int:
        """Blocks until the feed holds an update behind the cursor for one of `types` (acl_watch_wait: the blocking half of Watch.Recv,
        watch.go:38) -> the store's revision; raises AclError DEADLINE_EXCEEDED / CANCELLED by timeout_s / cancel (a ctypes c_int32)."""
        tids = [self.type_id(t) for t in types]
        if any(t < 0 for t in tids):
            raise AclError(ERR_FAILED_PRECONDITION, "unknown object type in watch request")
        arr = (C.c_int * max(1, len(tids)))(*tids)
        cur = C.c_uint64()
        opts = CallOpts(C.pointer(cancel) if cancel is not None else None, int((timeout_s or 0) * 1e9))
        self._check(self._L.acl_watch_wait(self._h, after_revision, arr, len(tids), C.byref(opts), C.byref(cur)))
        return cur.value

    def watch_recheck(self, after_revision: int, rtype, perm, stype, sid, srel=""):
        """RunWatch's loop body for a whole poll (watch.go:38-108): -> ([(revision, op, relationship 6-tuple, permissionship, err)], cursor):
        every update of `rtype` behind the cursor with the decision of ONE bulk Check `rtype:<its resource id>#perm@stype:sid[#srel]`."""
        out = []

        def cb(_u, rev, op, rp, perm_, err_):
            r = rp.contents
            out.append((rev, op, (r.resource_type.decode(), r.resource_id.decode(), r.relation.decode(), r.subject_type.decode(), r.subject_id.decode(),
                                  (r.subject_relation or b"").decode()), int(perm_), int(err_)))

        templ = CheckItem(_b(rtype), _b("-"), _b(perm), _b(stype), _b(sid), _b(srel))
        cur = C.c_uint64()
        self._check(self._L.acl_watch_recheck(self._h, after_revision, C.byref(templ), WATCH_CHECK_CB(cb), None, C.byref(cur)))
        return out, cur.value

    # ---- watch sets (include/aclgpu.h "watch sets": what every open watch gained or lost, whatever kind of write caused it)
    def watch_set(self, rt, perm, st, srel="") -> "WatchSet":
        """Opens a watch set for subjects `st[#srel]` against `rt#perm`.  An unknown type, permission or subject relation: FAILED_PRECONDITION."""
        sr = self.relation_id(st, srel)
        if srel and sr < 0:
            sr = -2  # (a relation that does not exist is not "no relation")
        out = C.c_void_p()
        self._check(self._L.acl_watch_set_open(self._h, self.type_id(rt), self.relation_id(rt, perm), self.type_id(st), sr, C.byref(out)))
        return WatchSet(self, out, rt)

    def subject_watch_set(self, rt, perm, st, srel="") -> "WatchSet":
        """Opens a SUBJECT-direction watch set: the watchers are resources of `rt` (WatchSet.add takes a resource id), the records' `resource_id` carries a
        subject id of `st`, and a record whose `reserved` is WATCH_CHANGE_WILDCARD reports the wildcard `st:*` instead of a concrete subject."""
        sr = self.relation_id(st, srel)
        if srel and sr < 0:
            sr = -2
        out = C.c_void_p()
        self._check(self._L.acl_watch_set_open_subjects(self._h, self.type_id(rt), self.relation_id(rt, perm), self.type_id(st), sr, C.byref(out)))
        return WatchSet(self, out, st)  # (the ids of its rows and records are of the subject type)

    # ---- paged lookups (include/aclgpu.h "paged lookups": limit and cursor, served from rows kept on the device)
    def _cursor(self, fn, rt, perm, st, srel, ids, row_type, cancel, timeout_s) -> "LookupCursor":
        sr = self.relation_id(st, srel)
        if srel and sr < 0:
            sr = -2  # (a relation that does not exist is not "no relation")
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        out = C.c_void_p()
        o = self._opts(cancel, timeout_s)
        self._check(fn(self._h, self.type_id(rt), self.relation_id(rt, perm), self.type_id(st), sr, ids.ctypes.data, ids.size, C.byref(o) if o else None, C.byref(out)))
        return LookupCursor(self, out, row_type, int(ids.size))

    def lookup_cursor(self, rt, perm, st, srel, subject_ids, cancel=None, timeout_s=None) -> "LookupCursor":
        """One walk now, pages later: row i holds the resources of `rt` that subject_ids[i] (`st[#srel]`) holds `perm` on, pinned at this revision."""
        return self._cursor(self._L.acl_lookup_cursor_open, rt, perm, st, srel, subject_ids, rt, cancel, timeout_s)

    def subjects_cursor(self, rt, perm, st, srel, resource_ids, cancel=None, timeout_s=None) -> "LookupCursor":
        """The other direction: row i holds the subjects `st[#srel]` that hold `perm` on resource_ids[i] of `rt` (LookupSubjects' named subjects)."""
        return self._cursor(self._L.acl_lookup_cursor_open_subjects, rt, perm, st, srel, resource_ids, st, cancel, timeout_s)

    # ---- derived cursors (include/aclgpu.h "derived lookup cursors": set algebra over rows kept on the device)
    def lookup_cursor_mixed(self, rt, perm, subjects, cancel=None, timeout_s=None) -> "LookupCursor":
        """lookup_cursor where every row names its own subject form: subjects = [(st, srel, id), ...]; row i is what lookup_ids_batch answers for
        subjects[i], all rows from one snapshot.  One walk per run of consecutive subjects of one form: sort them by form."""
        arr = np.zeros(len(subjects), dtype=SUBJECT_REF_DTYPE)
        form_ids = {}
        for i, (st, srel, sid) in enumerate(subjects):
            if (st, srel) not in form_ids:
                sr = self.relation_id(st, srel) if srel else -1
                form_ids[(st, srel)] = (self.type_id(st), -2 if srel and sr < 0 else sr)  # (a relation that does not exist is not "no relation")
            arr[i] = form_ids[(st, srel)] + (sid, 0)
        out = C.c_void_p()
        o = self._opts(cancel, timeout_s)
        self._check(self._L.acl_lookup_cursor_open_mixed(self._h, self.type_id(rt), self.relation_id(rt, perm), arr.ctypes.data, len(subjects), C.byref(o) if o else None,
                                                         C.byref(out)))
        return LookupCursor(self, out, rt, len(subjects))

    @staticmethod
    def _derive_args(srcs, exprs):
        """exprs = [(any, all, none), ...], each a list of (src, row) with src an index into srcs -> (handles, refs u32 [k, 2], exprs u32 [n, 4])"""
        handles = (C.c_void_p * max(len(srcs), 1))(*[s._c for s in srcs])
        if isinstance(exprs, tuple) and len(exprs) == 2 and isinstance(exprs[0], np.ndarray):  # (already packed: (refs, exprs) arrays)
            return handles, np.ascontiguousarray(exprs[0], dtype=np.uint32).reshape(-1, 2), np.ascontiguousarray(exprs[1], dtype=np.uint32).reshape(-1, 4)
        refs, recs = [], []
        for any_, all_, none in exprs:
            recs.append((len(refs), len(any_), len(all_), len(none)))
            refs += list(any_) + list(all_) + list(none)
        return handles, np.array(refs, dtype=np.uint32).reshape(-1, 2), np.array(recs, dtype=np.uint32).reshape(-1, 4)

    def derive_cursor(self, srcs, exprs, any_revision=False) -> "LookupCursor":
        """A NEW cursor whose row e is (union of any) & (intersection of all) & ~(union of none) over rows of the open cursors `srcs`:
        exprs = [(any, all, none), ...], each a list of (index into srcs, row); or the packed pair (refs [k, 2], exprs [n, 4]) of uint32 arrays.
        Computed on the device, two launches whatever the sizes; the sources may be closed afterwards."""
        handles, refs, recs = self._derive_args(srcs, exprs)
        out = C.c_void_p()
        self._check(self._L.acl_lookup_cursor_derive(self._h, handles, len(srcs), refs.ctypes.data, len(refs), recs.ctypes.data, len(recs),
                                                     DERIVE_ANY_REVISION if any_revision else 0, C.byref(out)))
        return LookupCursor(self, out, srcs[0].row_type if srcs else None, len(recs))

    def count_rows(self, srcs, exprs, any_revision=False) -> np.ndarray:
        """derive_cursor's evaluation with no row kept: -> the number of ids in every expression's row (u64 [n])"""
        handles, refs, recs = self._derive_args(srcs, exprs)
        counts = np.zeros(len(recs), dtype=np.uint64)
        self._check(self._L.acl_lookup_cursor_count(self._h, handles, len(srcs), refs.ctypes.data, len(refs), recs.ctypes.data, len(recs),
                                                    DERIVE_ANY_REVISION if any_revision else 0, counts.ctypes.data))
        return counts

    def principal_cursor(self, rt, perm, principals, cancel=None, timeout_s=None) -> "LookupCursor":
        """principals = [[(st, srel, name), ...], ...]: a user and the groups attached to it, as subject forms (an int in the place of a name is taken as
        the object's id).  One mixed open over every form of every principal plus one derive with an any-list per principal; -> the derived cursor,
        row p = the resources of `rt` principal p holds `perm` on."""
        forms = sorted({(st, srel or "", name) for p in principals for st, srel, name in p}, key=lambda f: (f[0], f[1]))  # (one run per subject form)
        index = {f: i for i, f in enumerate(forms)}
        subjects = [(st, srel, int(name) if isinstance(name, (int, np.integer)) else self.intern(st, name)) for st, srel, name in forms]
        with self.lookup_cursor_mixed(rt, perm, subjects, cancel, timeout_s) as src:
            return self.derive_cursor([src], [([(0, index[(st, srel or "", name)]) for st, srel, name in p], [], []) for p in principals])

    def selfcheck_subject_rows(self, rt, perm, st, srel, resource_ids) -> np.ndarray:
        """Test hook: the rows a subject-direction set would hold for these resource ids, by the set's device path -> [n, words] uint32."""
        rids = np.ascontiguousarray(resource_ids, dtype=np.uint32)
        words = max(1, (self.object_count(st) + 31) // 32)
        out = np.zeros((rids.size, words), dtype=np.uint32)
        self._check(self._L.acl_selfcheck_subject_rows(self._h, self.type_id(rt), self.relation_id(rt, perm), self.type_id(st), self.relation_id(st, srel) if srel else -1,
                                                       rids.ctypes.data, rids.size, out.ctypes.data, words))
        return out

    def _changes(self, recs, n):
        try:
            if not n:
                return np.zeros(0, dtype=WATCH_CHANGE_DTYPE)
            return np.ctypeslib.as_array(C.cast(recs, C.POINTER(C.c_uint32)), shape=(n * 4,)).copy().view(WATCH_CHANGE_DTYPE)
        finally:
            if recs:
                self._L.acl_free(recs)

    def selfcheck_rows_diff(self, old_rows: np.ndarray, new_rows: np.ndarray):
        """Test hook: the diff kernels alone on [n, old_words] / [n, new_words] uint32 rows -> records (WATCH_CHANGE_DTYPE; watcher = row)."""
        old_rows = np.ascontiguousarray(old_rows, dtype=np.uint32)
        new_rows = np.ascontiguousarray(new_rows, dtype=np.uint32)
        assert old_rows.ndim == new_rows.ndim == 2 and old_rows.shape[0] == new_rows.shape[0]
        recs, n = C.POINTER(WatchChange)(), C.c_size_t()
        self._check(self._L.acl_selfcheck_rows_diff(self._h, old_rows.ctypes.data, old_rows.shape[1], new_rows.ctypes.data, new_rows.shape[1], new_rows.shape[0],
                                                    C.byref(recs), C.byref(n)))
        return self._changes(recs, n.value)

    def batcher_start(self, max_items: int = 4096, max_wait_us: int = 200):
        self._check(self._L.acl_batcher_start(self._h, max_items, max_wait_us))

    def batcher_stop(self):
        self._check(self._L.acl_batcher_stop(self._h))

    def batcher_stats(self):
        b, i = C.c_uint64(), C.c_uint64()
        self._check(self._L.acl_batcher_stats(self._h, C.byref(b), C.byref(i)))
        return {"batches": b.value, "items": i.value}

    def check_one(self, rt, rid, perm, st, sid, srel="", cancel=None, timeout_s=None):
        """One CheckPermission (watch.go:50); rides the micro-batcher when it is running.  Blocks; releases the GIL."""
        it = CheckItem(*[_b(x if x is not None else "") for x in (rt, rid, perm, st, sid, srel)])
        p, e = C.c_uint8(), C.c_int32()
        o = self._opts(cancel, timeout_s)
        self._check(self._L.acl_check_one_opts(self._h, C.byref(it), C.byref(p), C.byref(e), C.byref(o) if o else None))
        return p.value, e.value

    def check_one_submit(self, rt, rid, perm, st, sid, srel="", tag=0):
        """acl_check_one without a blocked thread: returns at once; the answer arrives, tagged, through check_completions().
        This is the form a cgo shim binds (a goroutine parks on a channel, one poller drains the queue).  Needs a running batcher."""
        it = CheckItem(*[_b(x if x is not None else "") for x in (rt, rid, perm, st, sid, srel)])
        self._check(self._L.acl_check_one_submit(self._h, C.byref(it), int(tag)))

    def check_completions(self, max_items=256, timeout_s=-1.0):
        """Up to max_items answered submissions as (tag, rc, err, perm); blocks while there are none (timeout_s < 0: until one
        arrives, 0: never).  Releases the GIL."""
        buf = (Completion * max(1, max_items))()
        n = C.c_size_t()
        t = -1 if timeout_s < 0 else int(timeout_s * 1e9)
        self._check(self._L.acl_check_completions(self._h, buf, max_items, t, C.byref(n)))
        return [(int(buf[i].tag), int(buf[i].rc), int(buf[i].err), int(buf[i].perm)) for i in range(n.value)]

    def lookup_one_submit(self, rt, perm, st, sid, srel="", tag=0):
        """One LookupResources request WITHOUT a blocked thread (acl_lookup_one_submit): its answer arrives through lookup_completions."""
        self._check(self._L.acl_lookup_one_submit(self._h, _b(rt), _b(perm), _b(st), _b(sid), _b(srel or ""), int(tag)))

    def lookup_completions(self, rtype=None, max_items=64, timeout_s=-1.0):
        """Up to max_items answered lookups as (tag, rc, count, ids) -- ids = set of resource names when `rtype` is given, else the raw u32 bitmap;
        blocks while there are none (timeout_s < 0: until one arrives, 0: never).  Releases the GIL; frees the engine's rows."""
        from ._lib import LookupCompletion
        buf = (LookupCompletion * max(1, max_items))()
        n = C.c_size_t()
        t = -1 if timeout_s < 0 else int(timeout_s * 1e9)
        self._check(self._L.acl_lookup_completions(self._h, buf, max_items, t, C.byref(n)))
        out = []
        for i in range(n.value):
            c = buf[i]
            row = None
            if c.bitmap:
                row = np.ctypeslib.as_array(c.bitmap, shape=(max(1, c.words),)).copy()[:c.words]
                self._L.acl_free(c.bitmap)
            if row is not None and rtype is not None:
                ids = np.flatnonzero(np.unpackbits(row.view(np.uint8), bitorder="little"))
                row = {self.object_name(rtype, int(k)) for k in ids}
            out.append((int(c.tag), int(c.rc), int(c.count), row))
        return out

    def lookup_one(self, rt, perm, st, sid, srel="", cancel=None, timeout_s=None):
        """One LookupResources request (lookups.go:65) -> set of resource ids; concurrent callers with the same (type,
        permission, subject class) share one batched reverse walk while the batcher runs.  Blocks; releases the GIL.
        The result bitmap is engine-owned (acl_lookup_resources_alloc): no caller-side sizing race with concurrent writes."""
        bm, words, cnt = C.POINTER(C.c_uint32)(), C.c_size_t(), C.c_uint64()
        o = self._opts(cancel, timeout_s)
        self._check(self._L.acl_lookup_resources_alloc(self._h, _b(rt), _b(perm), _b(st), _b(sid), _b(srel or ""), C.byref(o) if o else None,
                                                       C.byref(bm), C.byref(words), C.byref(cnt)))
        try:
            a = np.ctypeslib.as_array(bm, shape=(words.value,)).copy()
        finally:
            self._L.acl_free(bm)
        ids = np.flatnonzero(np.unpackbits(a.view(np.uint8), bitorder="little"))
        return {self.object_name(rt, int(i)) for i in ids}

    def batcher_lookup_stats(self):
        w, n = C.c_uint64(), C.c_uint64()
        self._check(self._L.acl_batcher_lookup_stats(self._h, C.byref(w), C.byref(n)))
        return {"walks": w.value, "lookups": n.value}

    # ---- lookups
    def lookup_bitmap(self, rt, perm, st, sid, srel=""):
        words = (self.object_count(rt) + 1 + 31) // 32 + 1  # +1: the subject may be interned by the call
        bm = np.zeros(words, dtype=np.uint32)
        cnt = C.c_uint64()
        self._check(self._L.acl_lookup_resources(self._h, _b(rt), _b(perm), _b(st), _b(sid), _b(srel or ""), bm.ctypes.data, words, C.byref(cnt)))
        return bm, cnt.value

    def lookup(self, rt, perm, st, sid, srel=""):
        """-> set of resource ids (strings), as pkg/authz/lookups.go:129 collects them."""
        bm, _ = self.lookup_bitmap(rt, perm, st, sid, srel)
        ids = np.flatnonzero(np.unpackbits(bm.view(np.uint8), bitorder="little"))
        return {self.object_name(rt, int(i)) for i in ids}

    def lookup_ids_batch(self, rtype, perm, stype, srel, subject_ids, out=None):
        """n subjects of one class -> (bitmaps [n, words] u32, counts [n] u64).  `out` = a (bitmaps, counts) pair from an earlier call
        to write into (a caller in a loop: a fresh 0.8 MB array per call is ~200 page faults); the engine writes every word."""
        sids = np.ascontiguousarray(subject_ids, dtype=np.uint32)
        words = (self.object_count(rtype) + 31) // 32
        if out is not None and out[0].shape == (sids.size, max(1, words)) and out[0].dtype == np.uint32 and out[0].flags.c_contiguous \
                and out[1].shape == (sids.size,) and out[1].dtype == np.uint64:
            bms, counts = out
        else:
            bms = np.zeros((sids.size, max(1, words)), dtype=np.uint32)
            counts = np.zeros(sids.size, dtype=np.uint64)
        self._check(self._L.acl_lookup_resources_batch(self._h, self.type_id(rtype), self.relation_id(rtype, perm), self.type_id(stype),
                                                       self.relation_id(stype, srel), sids.ctypes.data, sids.size, bms.ctypes.data, max(1, words),
                                                       counts.ctypes.data))
        return bms, counts

    def lookup_ids(self, rtype, perm, stype, srel, subject_id):
        bms, _ = self.lookup_ids_batch(rtype, perm, stype, srel, [subject_id])
        return np.flatnonzero(np.unpackbits(bms[0].view(np.uint8), bitorder="little")).astype(np.uint32)

    def lookup_ids_multi(self, targets, stype, srel, subject_ids, cancel=None, timeout_s=None, out=None):
        """n subjects of one class against T targets [(rtype, perm), ...] in ONE reverse walk per subject (acl_lookup_resources_multi)
        -> (list of T arrays [n, words_j] u32, counts [n, T] u64).  Row (i, j) is what lookup_ids_batch answers for target j alone.
        `out` = the (rows, counts) pair of an earlier call with the same arguments, to write into (as lookup_ids_batch's)."""
        from ._lib import Target
        sids = np.ascontiguousarray(subject_ids, dtype=np.uint32)
        n, T = int(sids.size), len(targets)
        tg = (Target * max(1, T))()
        words = np.zeros(max(1, T), dtype=np.uintp)
        for j, (rt, pm) in enumerate(targets):
            tg[j].rtype, tg[j].permission = self.type_id(rt), self.relation_id(rt, pm)
            words[j] = (self.object_count(rt) + 31) // 32
        off = np.concatenate(([0], np.cumsum(words[:T]))).astype(np.int64)  # row j of a subject: [off[j], off[j + 1]) of its stride
        stride = int(off[T])
        flat = out[0][0].base if out is not None and T and stride else None  # (the rows are views of one [n, stride] array)
        if flat is not None and flat.shape == (n, stride) and flat.dtype == np.uint32 and flat.flags.c_contiguous and out[1].shape == (n, T) and out[1].dtype == np.uint64:
            counts = out[1]
        else:
            flat = np.zeros((n, max(1, stride)), dtype=np.uint32)
            counts = np.zeros((n, T), dtype=np.uint64)
        o = self._opts(cancel, timeout_s)
        self._check(self._L.acl_lookup_resources_multi(self._h, tg, T, self.type_id(stype), self.relation_id(stype, srel), sids.ctypes.data, n, flat.ctypes.data,
                                                       words.ctypes.data, counts.ctypes.data, C.byref(o) if o else None))
        return [flat[:, int(off[j]):int(off[j + 1])] for j in range(T)], counts

    def access_review(self, stype, sid, srel="", targets=None, cancel=None, timeout_s=None):
        """What one subject holds: {(rtype, perm): set of resource names}, every target answered by one reverse walk (acl_access_review).
        targets = [(rtype, perm), ...]; None: every relation and permission of every definition."""
        from ._lib import ReviewRow, Target
        tg, T = None, 0
        if targets is not None:
            T = len(targets)
            tg = (Target * max(1, T))()
            for j, (rt, pm) in enumerate(targets):
                tg[j].rtype, tg[j].permission = self.type_id(rt), self.relation_id(rt, pm)
        rows, nrows, bms = C.POINTER(ReviewRow)(), C.c_size_t(), C.POINTER(C.c_uint32)()
        o = self._opts(cancel, timeout_s)
        self._check(self._L.acl_access_review(self._h, _b(stype), _b(sid), _b(srel or ""), tg, T, C.byref(o) if o else None, C.byref(rows), C.byref(nrows), C.byref(bms)))
        try:
            out = {}
            for k in range(nrows.value):
                r = rows[k]
                a = np.ctypeslib.as_array(bms, shape=(r.row_off + max(1, r.row_words),))[r.row_off:r.row_off + r.row_words]
                rt = self.schema_name(r.rtype)
                ids = np.flatnonzero(np.unpackbits(a.view(np.uint8), bitorder="little"))
                out[(rt, self.schema_name(r.rtype, r.permission))] = {self.object_name(rt, int(i)) for i in ids}
        finally:
            self._L.acl_free(rows)
            self._L.acl_free(bms)
        return out

    # ---- LookupSubjects (not Workload.lookup_subjects: that is C3's list of LookupResources subjects)
    def lookup_subjects_ids_batch(self, rtype, perm, stype, srel, resource_ids, want_excluded=False, cancel=None, timeout_s=None):
        """n resources of one (type, permission) -> (bitmaps [n, words] u32 over the subject type's ids, counts [n] u64, flags [n] u8 (bit 0: a
        `stype:*` wildcard grants it)[, excluded [n, words] u32: who the wildcard leaves out, when want_excluded])."""
        rids = np.ascontiguousarray(resource_ids, dtype=np.uint32)
        words = max(1, (self.object_count(stype) + 31) // 32)
        bms = np.zeros((rids.size, words), dtype=np.uint32)
        counts = np.zeros(rids.size, dtype=np.uint64)
        flags = np.zeros(rids.size, dtype=np.uint8)
        ex = np.zeros((rids.size, words), dtype=np.uint32) if want_excluded else None
        o = self._opts(cancel, timeout_s)
        self._check(self._L.acl_lookup_subjects_batch(self._h, self.type_id(rtype), self.relation_id(rtype, perm), self.type_id(stype), self.relation_id(stype, srel),
                                                      rids.ctypes.data, rids.size, bms.ctypes.data, words, counts.ctypes.data, flags.ctypes.data,
                                                      ex.ctypes.data if ex is not None else None, C.byref(o) if o else None))
        return (bms, counts, flags, ex) if want_excluded else (bms, counts, flags)

    def lookup_subjects_bitmap(self, rt, rid, perm, st, srel="", want_excluded=True, cancel=None, timeout_s=None):
        """acl_lookup_subjects -> (bitmap u32, count, wildcard, excluded bitmap or None); the rows are the engine's (acl_free)."""
        bm, words, cnt, wild = C.POINTER(C.c_uint32)(), C.c_size_t(), C.c_uint64(), C.c_int()
        ex = C.POINTER(C.c_uint32)()
        o = self._opts(cancel, timeout_s)
        self._check(self._L.acl_lookup_subjects(self._h, _b(rt), _b(rid), _b(perm), _b(st), _b(srel or ""), C.byref(o) if o else None, C.byref(bm), C.byref(words),
                                                C.byref(cnt), C.byref(wild), C.byref(ex) if want_excluded else None))
        try:
            a = np.ctypeslib.as_array(bm, shape=(words.value,)).copy() if words.value else np.zeros(0, dtype=np.uint32)
            e = np.ctypeslib.as_array(ex, shape=(words.value,)).copy() if (want_excluded and bool(ex)) else None
        finally:
            self._L.acl_free(bm)
            if want_excluded and bool(ex):
                self._L.acl_free(ex)
        return a, cnt.value, bool(wild.value), e

    def lookup_subjects(self, rt, rid, perm, st, srel=""):
        """LookupSubjects(rt:rid#perm, subject type st[#srel]) -> (subject names, wildcard: bool, excluded names); names through acl_bitmap_names."""
        a, _, wild, e = self.lookup_subjects_bitmap(rt, rid, perm, st, srel)
        return set(self.bitmap_names(st, a)), wild, (set(self.bitmap_names(st, e)) if e is not None else set())

    # ---- Explain
    @staticmethod
    def _records(ptr, total, dtype):
        """A copy of the `total` records of `dtype` behind the engine's block `ptr` (the caller releases the block)."""
        return np.frombuffer(C.string_at(ptr, total * dtype.itemsize), dtype=dtype).copy() if total else np.zeros(0, dtype=dtype)

    def _explain_ids(self, fn, items, cancel, timeout_s, *record_ptrs):
        """One acl_explain*_bulk_ids call: `record_ptrs` receive the engine's blocks, one per offsets / records pair of the form, and stay the caller's to
        release -> (perm u8[n], err i32[n], flags u8[n], offsets u32[n + 1] per pair ...)."""
        items = np.ascontiguousarray(items, dtype=ITEM_DTYPE)
        n = items.size
        perm = np.zeros(max(1, n), dtype=np.uint8)
        err = np.zeros(max(1, n), dtype=np.int32)
        flags = np.zeros(max(1, n), dtype=np.uint8)
        offs = [np.zeros(n + 1, dtype=np.uint32) for _ in record_ptrs]
        outs = [a for off, ptr in zip(offs, record_ptrs) for a in (off.ctypes.data, C.byref(ptr))]
        o = self._opts(cancel, timeout_s)
        self._check(fn(self._h, items.ctypes.data, n, perm.ctypes.data, err.ctypes.data, flags.ctypes.data, *outs, C.byref(o) if o else None))
        return (perm[:n], err[:n], flags[:n], *offs)

    def _explain_one(self, fn, rt, rid, perm, st, sid, srel):
        """One acl_explain* call about one item in strings -> (permissionship, error code, flags, [the text's lines])."""
        it = CheckItem(*[_b(x if x is not None else "") for x in (rt, rid, perm, st, sid, srel)])
        p, e, f, txt = C.c_uint8(), C.c_int32(), C.c_uint32(), C.c_void_p()
        self._check(fn(self._h, C.byref(it), C.byref(p), C.byref(e), C.byref(f), C.byref(txt), None))
        try:
            lines = C.string_at(txt).decode().splitlines() if txt.value else []
        finally:
            self._L.acl_free(txt)
        return p.value, e.value, f.value, lines

    def explain_ids(self, items: np.ndarray, cancel=None, timeout_s=None):
        """acl_explain_bulk_ids: Check + a witness per granted item -> (perm u8[n], err i32[n], flags u8[n], hop_off u32[n + 1], hops HOP_DTYPE[]);
        item i's witness is hops[hop_off[i]:hop_off[i + 1]], a chain of stored relationships from its resource to its subject."""
        hp = C.POINTER(ExplainHop)()
        perm, err, flags, off = self._explain_ids(self._L.acl_explain_bulk_ids, items, cancel, timeout_s, hp)
        try:
            return perm, err, flags, off, self._records(hp, int(off[-1]), HOP_DTYPE)
        finally:
            self._L.acl_free(hp)

    def explain(self, rt, rid, perm, st, sid, srel=""):
        """acl_explain: (permissionship, error code, flags, [relationship strings in the tuple grammar of aclgpu/text.py])."""
        return self._explain_one(self._L.acl_explain, rt, rid, perm, st, sid, srel)

    def explain_proof_ids(self, items: np.ndarray, cancel=None, timeout_s=None):
        """acl_explain_proof_bulk_ids: Check + a proof per granted item, permissions with `-`, `&` and `.all()` included ->
        (perm u8[n], err i32[n], flags u8[n], hop_off u32[n + 1], hops HOP_DTYPE[], absent_off u32[n + 1], absent ITEM_DTYPE[]); item i rests on the stored
        relationships hops[hop_off[i]:hop_off[i + 1]] and on the Check items absent[absent_off[i]:absent_off[i + 1]], each of which answers NO."""
        hp, ap = C.POINTER(ExplainHop)(), C.c_void_p()
        perm, err, flags, off, aoff = self._explain_ids(self._L.acl_explain_proof_bulk_ids, items, cancel, timeout_s, hp, ap)
        try:
            return perm, err, flags, off, self._records(hp, int(off[-1]), HOP_DTYPE), aoff, self._records(ap, int(aoff[-1]), ITEM_DTYPE)
        finally:
            self._L.acl_free(hp)
            self._L.acl_free(ap)

    def explain_proof(self, rt, rid, perm, st, sid, srel=""):
        """acl_explain_proof: (permissionship, error code, flags, [lines]): the hops in the tuple grammar of aclgpu/text.py, then `not <goal>` per absence."""
        return self._explain_one(self._L.acl_explain_proof, rt, rid, perm, st, sid, srel)

    def explain_denial_ids(self, items: np.ndarray, cancel=None, timeout_s=None):
        """acl_explain_denial_bulk_ids: Check + the single writes that would grant each denied item -> (perm u8[n], err i32[n], flags u8[n],
        grant_off u32[n + 1], grants GRANT_DTYPE[]); writing grants[k] for k in grant_off[i]:grant_off[i + 1] with item i's subject grants item i."""
        gp = C.POINTER(Grant)()
        perm, err, flags, off = self._explain_ids(self._L.acl_explain_denial_bulk_ids, items, cancel, timeout_s, gp)
        total = int(off[-1])
        if not total:
            self._L.acl_free(gp)
            return perm, err, flags, off, np.zeros(0, dtype=GRANT_DTYPE)
        # No copy: the array reads the engine's allocation, which is released (acl_free) when the last array over it goes away -- 4 096 items about one
        # resource return 4 096 lists, tens of megabytes.
        buf = (C.c_char * (total * GRANT_DTYPE.itemsize)).from_address(C.addressof(gp.contents))
        weakref.finalize(buf, self._L.acl_free, C.c_void_p(C.addressof(gp.contents)))
        return perm, err, flags, off, np.frombuffer(buf, dtype=GRANT_DTYPE)

    def explain_denial(self, rt, rid, perm, st, sid, srel=""):
        """acl_explain_denial: (permissionship, error code, flags, [relationships to write, in the tuple grammar of aclgpu/text.py])."""
        return self._explain_one(self._L.acl_explain_denial, rt, rid, perm, st, sid, srel)

    def explain_revoke_ids(self, items: np.ndarray, cancel=None, timeout_s=None):
        """acl_explain_revoke_bulk_ids: Check + the single deletes that would revoke each granted item -> (perm u8[n], err i32[n], flags u8[n],
        cut_off u32[n + 1], cuts HOP_DTYPE[]); deleting cuts[k] for any one k in cut_off[i]:cut_off[i + 1] takes item i's grant away, no other single
        delete does."""
        cp = C.POINTER(ExplainHop)()
        perm, err, flags, off = self._explain_ids(self._L.acl_explain_revoke_bulk_ids, items, cancel, timeout_s, cp)
        try:
            return perm, err, flags, off, self._records(cp, int(off[-1]), HOP_DTYPE)
        finally:
            self._L.acl_free(cp)

    def explain_revoke(self, rt, rid, perm, st, sid, srel=""):
        """acl_explain_revoke: (permissionship, error code, flags, [relationships to delete, in the tuple grammar of aclgpu/text.py])."""
        return self._explain_one(self._L.acl_explain_revoke, rt, rid, perm, st, sid, srel)

    def selfcheck_denial_grants(self, rtype: str, member: str, stype: str, srel: str, states) -> np.ndarray:
        """Test hook (any engine): the host half of Explain denial on states [(object id, slot | level << 16)] -> GRANT_DTYPE records."""
        st = np.ascontiguousarray(states, dtype=np.uint32).reshape(-1, 2)
        gp, n = C.POINTER(Grant)(), C.c_size_t()
        self._check(self._L.acl_selfcheck_denial_grants(self._h, self.type_id(rtype), self.relation_id(rtype, member), self.type_id(stype), self.relation_id(stype, srel),
                                                        st.ctypes.data, st.shape[0], C.byref(gp), C.byref(n)))
        try:
            return self._records(gp, n.value, GRANT_DTYPE)
        finally:
            self._L.acl_free(gp)

    def selfcheck_explain_ops(self) -> np.ndarray:
        """Test hook (store-only engines): Explain's per-op side table, one EXPLAIN_OP_DTYPE record (acl_explain_op_t) per program op."""
        n = C.c_size_t()
        self._check(self._L.acl_selfcheck_explain_ops(self._h, None, 0, C.byref(n)))
        out = np.zeros(max(1, n.value), dtype=EXPLAIN_OP_DTYPE)
        self._check(self._L.acl_selfcheck_explain_ops(self._h, out.ctypes.data, n.value, C.byref(n)))
        return out[:n.value]

    def selfcheck_snapshot(self) -> bool:
        """Test hook (store-only engines): update + verify the host snapshot; True when the update was an in-place patch."""
        return self.selfcheck_snapshot_code() == 1

    def selfcheck_snapshot_code(self) -> int:
        """... 1: patched in place, 0: rebuilt, 2: the snapshot was current already."""
        p = C.c_int()
        self._check(self._L.acl_selfcheck_snapshot(self._h, C.byref(p)))
        return int(p.value)

    def selfcheck_json_array(self, body: bytes, arr_open: int, chunk_bytes: int = 0):
        """Test hook: the element spans of the JSON array at body[arr_open] as the list filters find them -> ([(begin, end)], offset of `]`)."""
        cap = max(1, len(body))
        spans = np.zeros(2 * cap, dtype=np.uint64)
        n, close = C.c_size_t(), C.c_size_t()
        self._check(self._L.acl_selfcheck_json_array(self._h, body, len(body), arr_open, chunk_bytes, spans.ctypes.data, cap, C.byref(n), C.byref(close)))
        return [(int(spans[2 * i]), int(spans[2 * i + 1])) for i in range(n.value)], close.value

    def selfcheck_compaction(self, phase: int) -> bool:
        """Test hook (store-only engines): phase 0 = build from a copy-on-write view; phase 1 = catch up, adopt, verify.
        Returns True when phase 1 adopted the background build."""
        a = C.c_int(1)
        self._check(self._L.acl_selfcheck_compaction(self._h, int(phase), C.byref(a)))
        return bool(a.value)

    def replica_calls(self):
        """[(HIP device ordinal, evaluations handed to that replica since open)]"""
        calls, devs = (C.c_uint64 * 64)(), (C.c_int32 * 64)()
        n = self._L.acl_replica_calls(self._h, calls, devs, 64)
        return [(int(devs[i]), int(calls[i])) for i in range(n)]

    # ---- measurement
    def stats(self) -> dict:
        s = Stats()
        self._check(self._L.acl_stats(self._h, C.byref(s)))
        out = {n: getattr(s, n) for n, _ in Stats._fields_}
        launches, ms = C.c_uint64(), C.c_double()  # (lookup cursors count on their own: acl_lookup_cursor_stats)
        self._check(self._L.acl_lookup_cursor_stats(self._h, C.byref(launches), C.byref(ms)))
        out["page_launches"], out["page_ms"] = launches.value, ms.value
        self._check(self._L.acl_lookup_derive_stats(self._h, C.byref(launches), C.byref(ms)))
        out["derive_launches"], out["derive_ms"] = launches.value, ms.value
        return out

    def stats_reset(self):
        self._check(self._L.acl_stats_reset(self._h))

    def set_timing(self, on: bool):
        self._check(self._L.acl_set_timing(self._h, 1 if on else 0))


class LookupCursor:
    """One acl_lookup_cursor_t: the rows of a batched lookup kept on the device, pinned at the revision of the open, read a page of ids at a time."""

    def __init__(self, engine: Engine, handle, row_type: str, n_rows: int):
        self._e, self._c, self.row_type, self.n_rows = engine, handle, row_type, n_rows

    def info(self):
        """-> (revision, counts [n] u64, flags [n] u8: SUBJECTS_WILDCARD on a subject cursor's rows)"""
        rev, n, rt = C.c_uint64(), C.c_uint32(), C.c_uint32()
        counts, flags = np.zeros(self.n_rows, dtype=np.uint64), np.zeros(self.n_rows, dtype=np.uint8)
        self._e._check(self._e._L.acl_lookup_cursor_info(self._e._h, self._c, C.byref(rev), C.byref(n), C.byref(rt), counts.ctypes.data, flags.ctypes.data))
        assert n.value == self.n_rows
        return rev.value, counts, flags

    def pages_raw(self, reqs, cancel=None, timeout_s=None):
        """reqs: [(row, after or None, limit), ...] -> (ids u32 [sum of limits], n u32 [m], more u8 [m]): request q's ids are
        ids[off[q]:off[q] + n[q]] with off the exclusive prefix of the limits, exactly as acl_lookup_cursor_pages leaves them."""
        m = len(reqs)
        arr = np.zeros((m, 4), dtype=np.uint32)
        for q, (row, after, limit) in enumerate(reqs):
            arr[q] = (row, PAGE_FROM_START if after is None else after, limit, 0)
        cap = int(arr[:, 2].sum(dtype=np.uint64))
        ids, n, more = np.zeros(max(cap, 1), dtype=np.uint32), np.zeros(m, dtype=np.uint32), np.zeros(m, dtype=np.uint8)
        o = Engine._opts(cancel, timeout_s)
        self._e._check(self._e._L.acl_lookup_cursor_pages(self._e._h, self._c, arr.ctypes.data, m, ids.ctypes.data, cap, n.ctypes.data, more.ctypes.data,
                                                          C.byref(o) if o else None))
        return ids[:cap], n, more

    def pages(self, reqs, cancel=None, timeout_s=None):
        """reqs: [(row, after or None, limit), ...] -> [(ids u32, more: bool), ...], all in ONE call (two kernel launches whatever len(reqs) is)"""
        ids, n, more = self.pages_raw(reqs, cancel, timeout_s)
        out, off = [], 0
        for q, (_row, _after, limit) in enumerate(reqs):
            out.append((ids[off:off + int(n[q])].copy(), bool(more[q])))
            off += int(limit)
        return out

    def page(self, row, after=None, limit=500):
        """-> (ids, more): the next `limit` ids of `row` behind `after` (None: from the start); continue with after = ids[-1] while more."""
        return self.pages([(row, after, limit)])[0]

    def page_names(self, row, after=None, limit=500, buf_bytes: int = 1 << 16):
        """-> (ids, names, more).  FAILED_PRECONDITION once an object id has been recycled since the open: reopen (page() keeps answering)."""
        ids, ends = np.zeros(limit, dtype=np.uint32), np.zeros(limit, dtype=np.uint32)
        buf = C.create_string_buffer(max(buf_bytes, 1024))
        n, more = C.c_uint32(), C.c_uint8()
        self._e._check(self._e._L.acl_lookup_cursor_page_names(self._e._h, self._c, int(row), PAGE_FROM_START if after is None else int(after), int(limit), ids.ctypes.data,
                                                               buf, len(buf), ends.ctypes.data, C.byref(n), C.byref(more)))
        raw, names, start = buf.raw, [], 0
        for k in range(n.value):
            names.append(raw[start:int(ends[k])].decode())
            start = int(ends[k])
        return ids[:n.value].copy(), names, bool(more.value)

    def close(self):
        if self._c is not None and getattr(self._e, "_h", None):
            c, self._c = self._c, None
            self._e._check(self._e._L.acl_lookup_cursor_close(self._e._h, c))
        self._c = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class WatchSet:
    """One acl_watch_set_t: the LookupResources rows of many watchers of one (type, permission), kept on the device between polls -- or, opened by
    Engine.subject_watch_set, the LookupSubjects rows of many watched resources.  `rtype` is the type of the ids in the rows and records."""

    def __init__(self, engine: Engine, handle, rtype: str):
        self._e, self._s, self._rt = engine, handle, rtype

    def add(self, sid: str, from_now: bool = False) -> int:
        """-> the watcher's id.  from_now: its baseline is what it holds at the next poll (nothing reported for it); else the empty row."""
        w = C.c_uint32()
        self._e._check(self._e._L.acl_watch_set_add(self._e._h, self._s, _b(sid), WATCHER_FROM_NOW if from_now else 0, C.byref(w)))
        return w.value

    def remove(self, w: int):
        self._e._check(self._e._L.acl_watch_set_remove(self._e._h, self._s, int(w)))

    def poll(self, cancel=None, timeout_s=None):
        """-> (revision, records): records is a WATCH_CHANGE_DTYPE array ordered by (watcher, resource_id); gained = 1, lost = 0."""
        recs, n, rev = C.POINTER(WatchChange)(), C.c_size_t(), C.c_uint64()
        o = Engine._opts(cancel, timeout_s)
        self._e._check(self._e._L.acl_watch_set_poll(self._e._h, self._s, C.byref(o) if o else None, C.byref(recs), C.byref(n), C.byref(rev)))
        return rev.value, self._e._changes(recs, n.value)

    def row(self, w: int) -> np.ndarray:
        """The watcher's row as of the last successful poll: sorted resource ids."""
        words = max(1, (self._e.object_count(self._rt) + 31) // 32)
        bm = np.zeros(words, dtype=np.uint32)
        self._e._check(self._e._L.acl_watch_set_row(self._e._h, self._s, int(w), bm.ctypes.data, words))
        return np.flatnonzero(np.unpackbits(bm.view(np.uint8), bitorder="little")).astype(np.uint32)

    def stats(self) -> dict:
        p, w, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._e._check(self._e._L.acl_watch_set_stats(self._e._h, self._s, C.byref(p), C.byref(w), C.byref(c)))
        return {"polls": p.value, "walks": w.value, "changes": c.value}

    def close(self):
        if self._s is not None and getattr(self._e, "_h", None):
            self._e._check(self._e._L.acl_watch_set_close(self._e._h, self._s))
        self._s = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

// engine.cpp -- C ABI of libaclgpu.so (include/aclgpu.h): open / close and the entry points themselves.  What they call lives by concern in
// engine_snapshot.cpp (snapshot upload, compaction, Eval), engine_pass.cpp (the forward passes), engine_intern.cpp (string <-> id plumbing),
// engine_lookup.cpp (LookupResources) and engine_keep.cpp (one-subject PostFilter by the reverse walk).
//
// Reference behaviour mirrored at this boundary:
//   CheckBulkPermissions : pairs are index-aligned with items (pkg/authz/check.go:54-57),
//                          per-item error or permissionship (check.go:55-63)
//   LookupResources      : set of ids with HAS_PERMISSION, order irrelevant (lookups.go:85-88,129)
//   every read is fully consistent (check.go:41-46): a write is visible to the next call.
// There is no CPU evaluation path: without a GPU acl_open() fails.
// Threading: engine_internal.hpp (state_mu / names_mu / PassCtx pool).
#include "engine_strings.hpp"

bool acl_engine::is_pinned(const void *p, size_t bytes) {
    if (!p) return false;
    std::lock_guard<std::mutex> lk(pinned_mu);
    const uintptr_t a = (uintptr_t)p;
    for (const auto &r : pinned)
        if (a >= r.first && a + bytes <= r.first + r.second) return true;
    return false;
}

extern "C" {

const char *acl_last_error(void) { return g_last_error.c_str(); }

int acl_open(const acl_config_t *cfg, acl_engine_t **out) { return acl_open_replicas(cfg, nullptr, 0, out); }

// The environment knobs (A/B and test switches; none is part of the product surface): read once per engine, here.
static void read_env_knobs(acl_engine *h) {
    if (const char *ev = getenv("ACL_SPIN_MAX")) h->spin_max = (uint32_t)std::max(0, atoi(ev));  // A/B knob
    if (const char *ev = getenv("ACL_REV_LOCAL")) h->rev_local = atoi(ev) != 0;
    if (const char *ev = getenv("ACL_REV_MULTI_MIN_T")) h->rev_multi_min_targets = (size_t)std::max(2, atoi(ev));      // A/B knobs (tools/lookup_multi_bench.py): where the
    if (const char *ev = getenv("ACL_REV_MULTI_MAX_WORDS")) h->rev_multi_max_words = (size_t)std::max(0, atoi(ev));    // many-target lookup takes its one walk
    if (const char *ev = getenv("ACL_REV_LDS_ROWS")) h->rev_lds_rows = atoi(ev) != 0;
    if (const char *ev = getenv("ACL_REV_SINK")) h->rev_sink_on = atoi(ev) != 0;
    if (const char *ev = getenv("ACL_REV_DEFER_MIN")) h->rev_defer_min = (uint32_t)std::max(1, atoi(ev));  // test knob: small graphs defer too
    if (const char *ev = getenv("ACL_REV_BIG_ROWS")) h->rev_big_rows = atoi(ev) != 0;  // A/B knob: 0 = rows beyond the LDS are walked, copied and cleared by ONE block (round 5)
    if (const char *ev = getenv("ACL_SHARD_A2A")) h->shard_a2a = atoi(ev) != 0;
    if (const char *ev = getenv("ACL_COMPACTION_SLACK")) h->compaction_slack = (uint64_t)std::max(0, atoi(ev));  // test knob (tools/fuzz_gpu.py --compact-early): small graphs compact too
    if (const char *ev = getenv("ACL_INTERN_THREADS")) h->intern_threads = (unsigned)std::min(64, std::max(2, atoi(ev)));  // A/B knob: host threads of bulk string interning
    if (const char *ev = getenv("ACL_LOCAL_CAP")) h->local_cap_limit = (uint32_t)std::max(256, atoi(ev));  // test knob: forces walks to overflow
    if (const char *ev = getenv("ACL_RAW_INTERN")) h->raw_intern = atoi(ev) != 0;  // test knob: acl_intern takes any bytes (the JSON scanners' decoding tests name objects no API request could)
    if (const char *ev = getenv("ACL_HOST_SPLIT")) h->host_split = (uint32_t)std::min(4, std::max(1, atoi(ev)));
    if (const char *ev = getenv("ACL_HOP2")) h->hop2_on = atoi(ev) != 0;  // A/B knob: 0 = the walk ignores the two-hop rows
    if (const char *ev = getenv("ACL_LOCAL_MAX")) h->local_max_items = (uint32_t)atoi(ev);  // A/B knob: 0 disables the single-launch path
}

int acl_open_replicas(const acl_config_t *cfg, const int32_t *devices, uint32_t n_devices, acl_engine_t **out) {
    if (!out) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_open: out is NULL");
    *out = nullptr;
    if (cfg && (cfg->flags & ACL_FLAG_STORE_ONLY)) {
        auto *so = new acl_engine();
        so->store_only = true;
        so->per_item_validation = (cfg->flags & ACL_FLAG_PER_ITEM_VALIDATION) != 0;
        so->lenient_lookup = (cfg->flags & ACL_FLAG_LENIENT_LOOKUP) != 0;
        read_env_knobs(so);  // (ACL_RAW_INTERN and ACL_INTERN_THREADS matter here; the device knobs set fields a store-only engine never reads)
        batcher_create(so);
        *out = so;
        return ACL_OK;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(ACL_ERR_UNAVAILABLE, "acl_open: no HIP device available (this engine has no CPU evaluation path)");
    auto h = std::make_unique<acl_engine>();
    h->per_item_validation = cfg && (cfg->flags & ACL_FLAG_PER_ITEM_VALIDATION) != 0;
    h->lenient_lookup = cfg && (cfg->flags & ACL_FLAG_LENIENT_LOOKUP) != 0;
    // the replicas: the device list of acl_open_replicas, else ACL_DEVICES="0,1,2,3" (a device may be named more than once: N logical replicas
    // on one GPU -- what the one-GPU test boxes exercise), else the one device of the config
    std::vector<int> list;
    if (devices && n_devices) list.assign(devices, devices + n_devices);
    else if (const char *ev = getenv("ACL_DEVICES")) {
        for (const char *q = ev; *q;) {
            char *end = nullptr;
            const long v = std::strtol(q, &end, 10);
            if (end == q) break;
            list.push_back((int)v);
            q = *end == ',' ? end + 1 : end;
        }
    }
    if (list.empty()) list.push_back(cfg ? cfg->device : -1);
    if (list.size() > 64) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_open: at most 64 replicas");
    for (size_t i = 0; i < list.size(); i++) {
        int dev = list[i];
        if (dev < 0) {
            if (hipGetDevice(&dev) != hipSuccess) dev = 0;
        }
        if (dev >= ndev) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_open: device ordinal out of range");
        auto d = std::make_unique<DevState>();
        d->device = dev;
        d->index = (int)i;
        hipError_t e = hipSetDevice(dev);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&d->up_stream, hipStreamNonBlocking);
        if (e != hipSuccess) return fail(ACL_ERR_UNAVAILABLE, std::string("acl_open: ") + hipGetErrorString(e));
        d->grid_blocks = expand_grid_blocks(dev);
        d->local_blocks = local_grid_blocks(dev, 2048);  // (refined per snapshot: ensure_snapshot)
        d->local_blocks_wide = local_grid_blocks(dev, 2048, true);
        h->devs.push_back(std::move(d));
    }
    if (cfg && cfg->max_sub_batch) h->max_sub_batch = cfg->max_sub_batch;
    if (cfg && cfg->frontier_entries) h->cfg_frontier_entries = cfg->frontier_entries;
    if (cfg && cfg->contexts) h->max_ctx = std::min<uint32_t>(cfg->contexts, 16);
    read_env_knobs(h.get());  // (after the cfg fields, where ACL_LOCAL_MAX has always been read)
    // the first context of every replica is created here, so that "out of device memory" surfaces at open
    for (auto &d : h->devs) {
        std::unique_ptr<PassCtx> c0;
        int rc = new_ctx(h.get(), d.get(), &c0, 0);
        if (rc) return rc;
        d->free_ctxs.push_back(c0.get());
        d->ctxs.push_back(std::move(c0));
        // ACL_FLAG_EAGER_CONTEXTS: every context of the pool now -- a context made on demand costs its caller (and, under pool_mu, every caller that
        // arrives meanwhile) the allocation of its frontier buffers and pinned staging, milliseconds into the first request that finds the pool busy
        for (uint32_t k = 1; cfg && (cfg->flags & ACL_FLAG_EAGER_CONTEXTS) && k < h->max_ctx; k++) {
            std::unique_ptr<PassCtx> ck;
            rc = new_ctx(h.get(), d.get(), &ck, (int)k);
            if (rc) return rc;
            d->free_ctxs.insert(d->free_ctxs.begin(), ck.get());  // (behind the first one: the pool hands out the context released last)
            d->ctxs.push_back(std::move(ck));
        }
    }
    (void)hipSetDevice(h->dev0().device);
    batcher_create(h.get());
    *out = h.release();
    return ACL_OK;
}

void acl_close(acl_engine_t *h) {
    if (!h) return;
    (void)acl_batcher_stop(h);
    async_shutdown(h);
    batcher_destroy(h);
    intern_pool_destroy(h);
    (void)acl_shard_rccl_destroy(h);
    compaction_join(h);
    watch_sets_release(h);
    lookup_cursors_release(h);
    if (h->store_only) {
        delete h;
        return;
    }
    {
        std::lock_guard<RwLock> lk(h->state_mu);  // waits for evaluations in flight
        for (auto &d : h->devs) {
            (void)hipSetDevice(d->device);
            d->ctxs.clear();
        }
        (void)hipSetDevice(h->dev0().device);
        h->shard_ctx.reset();
        if (h->compaction)
            for (auto &pd : h->compaction->per)
                if (pd->stream) {
                    (void)hipSetDevice(pd->device);
                    (void)hipStreamDestroy(pd->stream);
                }
        h->compaction.reset();
        std::lock_guard<std::mutex> plk(h->pinned_mu);
        for (auto &r : h->pinned) (void)hipHostFree((void *)r.first);
        h->pinned.clear();
    }
    std::vector<std::pair<int, hipStream_t>> ups;
    for (auto &d : h->devs) ups.emplace_back(d->device, d->up_stream);
    delete h;  // (frees the replicas' arrays: hipFree takes pointers of any device)
    for (auto &u : ups)
        if (u.second) {
            (void)hipSetDevice(u.first);
            (void)hipStreamDestroy(u.second);
        }
}

int acl_load_bootstrap(acl_engine_t *h, const char *schema, size_t schema_len, const char *rels, size_t rels_len) {
    std::lock_guard<RwLock> lk(h->state_mu);
    std::unique_lock<std::shared_mutex> nlk(h->names_mu);
    if (!schema) return fail(ACL_ERR_INVALID_ARGUMENT, "schema is NULL");
    compaction_join(h);  // a background build of the OLD schema's graph: wait for it and drop it (its ids mean nothing from here on)
    Status s = h->store.load_schema(std::string(schema, schema_len));
    if (!s.ok()) return fail(s);
    h->snap_valid = false;
    h->set_dev_valid(false);
    h->set_rev_uploaded(false);
    if (rels && rels_len) {
        s = h->store.load_relationship_lines(std::string(rels, rels_len));
        if (!s.ok()) return fail(s);
    }
    return ACL_OK;
}

int acl_type_id(acl_engine_t *h, const char *type) {
    std::shared_lock<std::shared_mutex> nlk(h->names_mu);
    return type ? h->store.schema().type_of(type) : -1;
}
int acl_relation_id(acl_engine_t *h, int type, const char *name) {
    std::shared_lock<std::shared_mutex> nlk(h->names_mu);
    const Schema &sc = h->store.schema();
    if (!name || type < 0 || type >= (int)sc.defs.size()) return -1;
    return sc.defs[type].find(name);
}
int acl_intern(acl_engine_t *h, int type, const char *object_id, uint32_t *id_out) {
    std::shared_lock<RwLock> slk(h->state_mu);
    std::unique_lock<std::shared_mutex> nlk(h->names_mu);
    const Schema &sc = h->store.schema();
    if (empty(object_id) || !id_out || type < 0 || type >= (int)sc.defs.size()) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_intern: bad argument");
    if (!h->raw_intern && !valid_object_id(object_id)) return fail(ACL_ERR_INVALID_ARGUMENT, std::string("acl_intern: `") + object_id + "` does not match the API's object id pattern");  // (validate.hpp: names in the tables are well-formed)
    *id_out = h->store.intern_object(type, object_id, true);  // (the caller keeps this id: never recycled)
    return ACL_OK;
}
int acl_find(acl_engine_t *h, int type, const char *object_id, uint32_t *id_out) {
    std::shared_lock<std::shared_mutex> nlk(h->names_mu);
    const Schema &sc = h->store.schema();
    if (empty(object_id) || !id_out || type < 0 || type >= (int)sc.defs.size()) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_find: bad argument");
    if (!h->store.objects(type).find(object_id, id_out)) return fail(ACL_ERR_NOT_FOUND, "object not found");
    h->store.touch(type, *id_out);  // (the id is the caller's for the length of a quarantine: an unreferenced object is not renamed under it)
    return ACL_OK;
}
int64_t acl_object_name_copy(acl_engine_t *h, int type, uint32_t id, char *buf, size_t cap) {
    std::shared_lock<std::shared_mutex> nlk(h->names_mu);
    const Schema &sc = h->store.schema();
    if (type < 0 || type >= (int)sc.defs.size()) return -1;
    const std::string *n = h->store.objects(type).name(id);
    if (!n) return -1;
    if (buf && cap) {
        const size_t k = std::min(n->size(), cap - 1);
        std::memcpy(buf, n->data(), k);
        buf[k] = 0;
    }
    return (int64_t)n->size();
}
// The names behind a LookupResources bitmap, a block per call (the shim's stream, lookups.go:75-83: one cgo call and one turn at the names lock per BLOCK of results,
// not per result).
int acl_bitmap_names(acl_engine_t *h, int type, const uint32_t *bitmap, size_t words, uint64_t *cursor, char *buf, size_t cap, uint32_t *ends, size_t max_names, size_t *n_out) {
    if (!cursor || !n_out || (words && !bitmap) || !buf || !ends || cap < 1024 || cap > 0xFFFFFFFFull || !max_names)
        return fail(ACL_ERR_INVALID_ARGUMENT, "acl_bitmap_names: bad argument (buf must hold at least 1024 bytes: the longest object id)");
    std::shared_lock<std::shared_mutex> nlk(h->names_mu);
    const Schema &sc = h->store.schema();
    if (type < 0 || type >= (int)sc.defs.size()) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_bitmap_names: unknown object type");
    const ObjectTable &ot = h->store.objects(type);
    size_t n = 0, used = 0;
    uint64_t bit = *cursor;
    const uint64_t nbits = (uint64_t)words * 32;
    while (bit < nbits && n < max_names) {
        const uint32_t wv = bitmap[bit >> 5] >> (bit & 31u);
        if (!wv) {
            bit = (bit | 31u) + 1;
            continue;
        }
        bit += (uint64_t)__builtin_ctz(wv);
        const std::string *nm = ot.name((uint32_t)bit);  // (an id that lost its name meanwhile, or an anonymous bulk-loaded one: an empty name, as the per-id call's -1)
        const size_t len = nm ? nm->size() : 0;
        if (used + len > cap) break;  // (the next call starts here: cap >= the longest id, so a call always makes progress)
        if (len) std::memcpy(buf + used, nm->data(), len);
        used += len;
        ends[n++] = (uint32_t)used;
        bit++;
    }
    *cursor = bit;
    *n_out = n;
    return ACL_OK;
}
const char *acl_object_name(acl_engine_t *h, int type, uint32_t id) {
    std::shared_lock<std::shared_mutex> nlk(h->names_mu);
    const Schema &sc = h->store.schema();
    if (type < 0 || type >= (int)sc.defs.size()) return nullptr;
    const std::string *n = h->store.objects(type).name(id);
    return n ? n->c_str() : nullptr;
}
uint32_t acl_object_count(acl_engine_t *h, int type) {
    std::shared_lock<std::shared_mutex> nlk(h->names_mu);
    const Schema &sc = h->store.schema();
    if (type < 0 || type >= (int)sc.defs.size()) return 0;
    return h->store.objects(type).count();
}

int acl_write(acl_engine_t *h, const acl_update_t *ups, int n, const acl_filter_t *pre, int m, uint64_t *rev) {
    if (n < 0 || m < 0 || (n && !ups) || (m && !pre)) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_write: bad argument");
    std::vector<UpdateText> u(n);
    for (int i = 0; i < n; i++) {
        const acl_relationship_t &r = ups[i].rel;
        u[i].op = ups[i].op;
        u[i].rel.rtype = r.resource_type ? r.resource_type : "";
        u[i].rel.rid = r.resource_id ? r.resource_id : "";
        u[i].rel.rel = r.relation ? r.relation : "";
        u[i].rel.stype = r.subject_type ? r.subject_type : "";
        u[i].rel.sid = r.subject_id ? r.subject_id : "";
        u[i].rel.srel = r.subject_relation ? r.subject_relation : "";
        u[i].rel.expires_at = r.expires_at;
    }
    std::vector<FilterText> p(m);
    for (int i = 0; i < m; i++) p[i] = to_filter(&pre[i]);
    std::lock_guard<RwLock> lk(h->state_mu);
    std::unique_lock<std::shared_mutex> nlk(h->names_mu);
    Status s = h->store.write(u, p, rev);
    if (s.ok()) h->feed_wake();  // (acl_watch_wait)
    return s.ok() ? ACL_OK : fail(s);
}

int acl_delete_by_filter(acl_engine_t *h, const acl_filter_t *f, uint64_t *n_deleted, uint64_t *rev) {
    return acl_delete_by_filter_pre(h, f, nullptr, 0, n_deleted, rev);
}

// DeleteRelationships with OptionalPreconditions: evaluated against the pre-delete state, atomically with the delete
int acl_delete_by_filter_pre(acl_engine_t *h, const acl_filter_t *f, const acl_filter_t *pre, int n_pre, uint64_t *n_deleted, uint64_t *rev) {
    if (!f) return fail(ACL_ERR_INVALID_ARGUMENT, "filter is NULL");
    if (n_pre < 0 || (n_pre && !pre)) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_delete_by_filter_pre: bad argument");
    std::vector<FilterText> p(n_pre);
    for (int i = 0; i < n_pre; i++) p[i] = to_filter(&pre[i]);
    std::lock_guard<RwLock> lk(h->state_mu);
    std::unique_lock<std::shared_mutex> nlk(h->names_mu);
    if (n_pre) {
        Status ps = h->store.check_preconditions(p);
        if (!ps.ok()) return fail(ps);
    }
    Status s = h->store.delete_by_filter(to_filter(f), n_deleted, rev);
    if (s.ok()) h->feed_wake();
    return s.ok() ? ACL_OK : fail(s);
}

int acl_read(acl_engine_t *h, const acl_filter_t *f, acl_read_cb cb, void *user) {
    if (!f || !cb) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_read: bad argument");
    std::lock_guard<RwLock> lk(h->state_mu);  // the scan settles pending bulk appends: exclusive
    Status s = h->store.read(to_filter(f), [&](const RelText &r) {
        acl_relationship_t o{r.rtype.c_str(), r.rid.c_str(), r.rel.c_str(), r.stype.c_str(), r.sid.c_str(), r.srel.c_str(), r.expires_at};
        cb(user, &o);
    });
    return s.ok() ? ACL_OK : fail(s);
}

int acl_add_edges(acl_engine_t *h, int rtype, int rel, int stype, int srel, size_t n, const uint32_t *res, const uint32_t *subj) {
    std::lock_guard<RwLock> lk(h->state_mu);
    std::unique_lock<std::shared_mutex> nlk(h->names_mu);
    Status s = h->store.add_edges(rtype, rel, stype, srel, n, res, subj);
    return s.ok() ? ACL_OK : fail(s);
}

uint64_t acl_revision(acl_engine_t *h) {
    std::shared_lock<RwLock> lk(h->state_mu);
    return h->store.revision();
}
int acl_set_now(acl_engine_t *h, int64_t t) {
    std::lock_guard<RwLock> lk(h->state_mu);
    h->store.set_now(t);
    return ACL_OK;
}
int acl_snapshot(acl_engine_t *h) {
    std::lock_guard<RwLock> lk(h->state_mu);
    return ensure_snapshot(h);  // (sets the device of every replica it uploads to)
}

int acl_replica_calls(acl_engine_t *h, uint64_t *calls_out, int32_t *devices_out, uint32_t cap) {
    std::lock_guard<std::mutex> lk(h->pool_mu);
    for (uint32_t i = 0; i < cap && i < h->devs.size(); i++) {
        if (calls_out) calls_out[i] = h->devs[i]->calls;
        if (devices_out) devices_out[i] = h->devs[i]->device;
    }
    return (int)h->devs.size();
}

void *acl_stream(acl_engine_t *h) { return (h->devs.empty() || h->dev0().ctxs.empty()) ? nullptr : (void *)h->dev0().ctxs[0]->stream; }
int acl_sync(acl_engine_t *h) {
    if (h->store_only) return fail(ACL_ERR_UNAVAILABLE, "engine was opened store-only (no GPU): Check / LookupResources are unavailable");
    std::vector<std::pair<int, hipStream_t>> ss;
    {
        std::lock_guard<std::mutex> lk(h->pool_mu);
        for (auto &d : h->devs)
            for (auto &c : d->ctxs) ss.emplace_back(d->device, c->stream);
    }
    for (auto &s : ss) {
        HIP_TRY(hipSetDevice(s.first));
        HIP_TRY(hipStreamSynchronize(s.second));
    }
    return ACL_OK;
}

int acl_check_bulk_ids_device(acl_engine_t *h, const void *d_items, size_t n, void *d_perm_out, void *d_err_out) {
    if (n && (!d_items || !d_perm_out)) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_check_bulk_ids_device: NULL buffer");
    Eval ev;
    int rc = ev.begin(h, false, CallOpts(), -1, device_of(h, d_perm_out));  // (a replica on the device the caller's buffers live on)
    if (rc) return rc;
    rc = check_device(h, ev.c, (const uint4 *)d_items, n, (uint8_t *)d_perm_out, (int32_t *)d_err_out);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(ev.c->stream));
    ev_collect(ev.c);
    return ACL_OK;
}

int acl_check_bulk_ids(acl_engine_t *h, const acl_item_t *items, size_t n, uint8_t *perm_out, int32_t *err_out) {
    return acl_check_bulk_ids_opts(h, items, n, perm_out, err_out, nullptr);
}

int acl_check_bulk_ids_opts(acl_engine_t *h, const acl_item_t *items, size_t n, uint8_t *perm_out, int32_t *err_out, const acl_call_opts_t *o) {
    if (n && (!items || !perm_out)) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_check_bulk_ids: NULL buffer");
    const CallOpts opts = call_opts(o);
    if (!n) return h->store_only ? fail(ACL_ERR_UNAVAILABLE, "engine was opened store-only (no GPU): Check / LookupResources are unavailable") : ACL_OK;
    Eval ev;
    int rc = ev.begin(h, false, opts);
    if (rc) return rc;
    return check_ids_host(h, ev.c, items, n, perm_out, err_out);
}

int acl_check_bulk(acl_engine_t *h, const acl_check_item_t *items, size_t n, uint8_t *perm_out, int32_t *err_out) {
    if (n && (!items || !perm_out || !err_out)) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_check_bulk: NULL buffer");
    return check_bulk_strings(h, CStrItems{items}, n, perm_out, err_out);
}

// the same with {pointer, length} fields: no strlen per field, and no NUL needed behind the bytes -- a cgo shim points at Go string data
int acl_check_bulk_v(acl_engine_t *h, const acl_check_item_v_t *items, size_t n, uint8_t *perm_out, int32_t *err_out) {
    if (n && (!items || !perm_out || !err_out)) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_check_bulk_v: NULL buffer");
    return check_bulk_strings(h, ViewItems{items}, n, perm_out, err_out);
}

int acl_check_bulk_packed(acl_engine_t *h, const acl_packed_request_t *req, uint8_t *perm_out, int32_t *err_out, const acl_call_opts_t *opts) {
    return check_bulk_packed_call(h, req, perm_out, err_out, opts);
}
int acl_check_bulk_keep_packed(acl_engine_t *h, const acl_packed_request_t *req, const uint32_t *item_off, size_t k_items, uint8_t *keep_out) {
    return check_bulk_keep_packed_call(h, req, item_off, k_items, keep_out);
}
int acl_check_bulk_keep_v(acl_engine_t *h, const acl_check_item_v_t *items, size_t n, const uint32_t *item_off, size_t k_items, uint8_t *keep_out) {
    return check_bulk_keep_v_call(h, items, n, item_off, k_items, keep_out);
}

// names -> the 16-byte items of the id entry points, in bulk and without a device pass (works on a store-only engine)
int acl_resolve_bulk_v(acl_engine_t *h, const acl_check_item_v_t *items, size_t n, acl_item_t *out, int32_t *err_out) {
    if (n && (!items || !out || !err_out)) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_resolve_bulk_v: NULL buffer");
    std::vector<std::pair<uint32_t, int32_t>> bad;
    {
        std::shared_lock<std::shared_mutex> nlk(h->names_mu);
        if (!h->store.has_schema()) return fail(ACL_ERR_FAILED_PRECONDITION, "no schema loaded");
        intern_items(h, ViewItems{items}, n, out, &bad, true);
    }
    if (n) std::memset(err_out, 0, n * sizeof(int32_t));
    for (const auto &be : bad) err_out[be.first] = be.second;
    return ACL_OK;
}

int acl_check_bulk_v_opts(acl_engine_t *h, const acl_check_item_v_t *items, size_t n, uint8_t *perm_out, int32_t *err_out, const acl_call_opts_t *opts) {
    if (n && (!items || !perm_out || !err_out)) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_check_bulk_v_opts: NULL buffer");
    return check_bulk_strings(h, ViewItems{items}, n, perm_out, err_out, opts);
}

int acl_lookup_resources_batch(acl_engine_t *h, int rtype, int perm, int stype, int srel, const uint32_t *sids, size_t n, uint32_t *bitmaps,
                               size_t words, uint64_t *counts) {
    return lookup_batch_call(h, rtype, perm, stype, srel, sids, n, bitmaps, words, counts, CallOpts());
}

int acl_lookup_resources_ids(acl_engine_t *h, int rtype, int perm, int stype, int srel, uint32_t sid, uint32_t *bitmap, size_t words, uint64_t *count) {
    return acl_lookup_resources_batch(h, rtype, perm, stype, srel, &sid, 1, bitmap, words, count);
}

int acl_lookup_resources(acl_engine_t *h, const char *rtype, const char *perm, const char *stype, const char *sid, const char *srel, uint32_t *bitmap,
                         size_t words, uint64_t *count) {
    return lookup_opts_call(h, rtype, perm, stype, sid, srel, bitmap, words, count, CallOpts());
}

// LookupResources with an engine-owned result: the bitmap is sized by the engine at the moment of the walk, so a racing
// WriteRelationships that interns new objects of the type cannot make the caller's buffer "too small" (advice r1).
int acl_lookup_resources_alloc(acl_engine_t *h, const char *rtype, const char *perm, const char *stype, const char *sid, const char *srel,
                               const acl_call_opts_t *o, uint32_t **bitmap_out, size_t *words_out, uint64_t *count_out) {
    if (!bitmap_out || !words_out) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_lookup_resources_alloc: NULL output");
    *bitmap_out = nullptr;
    *words_out = 0;
    const CallOpts opts = call_opts(o);
    int rt, pm, st, sr;
    uint32_t sub;
    int rc = resolve_lookup(h, rtype, perm, stype, sid, srel, &rt, &pm, &st, &sr, &sub);
    if (rc) return rc;
    return owned_bitmap_retry("lookup: the object table kept growing faster than the result bitmap", [&]() -> int {
        const size_t words = owned_bitmap_words(h, rt);
        uint32_t *bm = nullptr;
        int rc = result_block(words, "out of host memory for the result bitmap", &bm);
        if (rc) return rc;
        rc = lookup_one_routed(h, rt, pm, st, sr, sub, bm, words, count_out, opts);
        if (rc == ACL_OK) {
            *bitmap_out = bm;
            *words_out = words;
        } else {
            std::free(bm);
        }
        return rc;
    });
}
void acl_free(void *p) { std::free(p); }

int acl_stats(acl_engine_t *h, acl_stats_t *out) {
    if (!out) return fail(ACL_ERR_INVALID_ARGUMENT, "out is NULL");
    uint64_t recycled;
    {
        std::shared_lock<std::shared_mutex> nlk(h->names_mu);
        recycled = h->store.ids_recycled();
    }
    std::lock_guard<std::mutex> lk(h->stats_mu);
    *out = h->stats;
    out->ids_recycled = recycled;
    out->keep_route_calls = h->keep_route_calls.load(std::memory_order_relaxed);
    out->depth_sweeps = h->depth_sweeps.load(std::memory_order_relaxed);
    out->hop2_rows = h->hop2_rows_now.load(std::memory_order_relaxed);
    return ACL_OK;
}
int acl_stats_reset(acl_engine_t *h) {
    std::lock_guard<std::mutex> lk(h->stats_mu);
    uint64_t e = h->stats.snapshot_edges, b = h->stats.snapshot_bytes, el = h->stats.snapshot_edges_local;
    uint64_t sb = h->stats.snapshot_builds, sp = h->stats.snapshot_patches;
    h->stats = acl_stats_t{};
    h->stats.snapshot_builds = sb;
    h->stats.snapshot_patches = sp;
    h->stats.snapshot_edges_local = el;
    h->stats.snapshot_edges = e;
    h->stats.snapshot_bytes = b;
    h->page_launches = 0;
    h->page_ms = 0;
    h->derive_launches = 0;
    h->derive_ms = 0;
    return ACL_OK;
}
int acl_set_timing(acl_engine_t *h, int on) {
    h->timing.store(on != 0);
    return ACL_OK;
}

}  // extern "C"

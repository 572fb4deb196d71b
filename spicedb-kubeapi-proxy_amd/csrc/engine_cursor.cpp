// engine_cursor.cpp -- lookup cursors (include/aclgpu.h "paged lookups"): the limit and cursor of LookupResources / LookupSubjects.
//
// Open is one ordinary evaluation (state_mu shared + a context of the pool, as a watch set's poll): the n rows of the batch call are produced straight into
// the cursor's device array (lookup_batch with a device destination, subjects_walk_device; a permission with `-` / `&` / `.all()` is confirmed on host rows
// and uploaded once, as watch sets do it), and the rank index is built over them once: the diff's count + scan against an empty old array, offs[row][tile] =
// set bits in front of the tile.  The row counts are differences of that index.
// A page takes no snapshot and no context: the rows are the cursor's own and never change, so the call needs the cursor's mutex, its stream and its scratch
// only -- one upload of the requests, two launches (kernels.hip k_rows_page_plan, k_rows_page), one copy back of the counts and of the written ids.
// What pins the answer: the rows (a copy, not a view of the snapshot), the revision read at the open, the row width of the open (ids interned later have no
// bit).  What expires it: a schema reload (Store::schema_loads) for every call, a recycled id (Store::ids_recycled) for the calls that return names.
#include "engine_internal.hpp"

struct acl_lookup_cursor {
    std::mutex mu;
    int rtype = 0, perm = 0, stype = 0, srel = -1;
    bool subjects = false;  // the rows are LookupSubjects rows of resources (bits: subject ids of stype)
    int row_type() const { return subjects ? stype : rtype; }
    int device = 0;  // HIP ordinal the rows live on
    size_t n_rows = 0, row_words = 0, bytes = 0;
    uint32_t ntiles = 0;
    uint64_t revision = 0, schema_loads = 0, ids_recycled = 0;
    DevArray<uint32_t> rows;
    DevArray<uint64_t> offs;  // [n_rows * ntiles + 1]
    std::vector<uint64_t> counts;
    std::vector<uint8_t> flags;
    // a page call's own: stream, scratch, staging, one event pair
    hipStream_t stream = nullptr;
    DevArray<uint4> d_reqs;
    DevArray<ulonglong2> d_plan;
    DevArray<uint32_t> d_res, d_ids;
    PinnedBuf h_in, h_out;
    hipEvent_t ev[2] = {nullptr, nullptr};
    ~acl_lookup_cursor() {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamDestroy(stream);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

namespace aclint {

constexpr size_t kCursorBytes = (size_t)1 << 30;      // the rows of all open cursors of an engine, at most
constexpr uint64_t kPageMaxIds = 1ull << 28;          // the limits of one pages call, summed, at most
constexpr uint64_t kPageOneCopyIds = 16384;           // up to this many ids asked for, the ids travel with the counts (one synchronisation instead of two)

static int cursor_args_ok(acl_engine *h, int rtype, int perm, int stype, int srel) {
    if (!h->store.has_schema()) return fail(ACL_ERR_FAILED_PRECONDITION, "no schema loaded");
    const Schema &sc = h->store.schema();
    if (rtype < 0 || rtype >= (int)sc.defs.size() || stype < 0 || stype >= (int)sc.defs.size() || perm < 0 || perm >= (int)sc.defs[rtype].members.size() || srel < -1 ||
        srel >= (int)sc.defs[stype].members.size())
        return fail(ACL_ERR_FAILED_PRECONDITION, "lookup cursor: unknown type, permission or subject relation");
    return ACL_OK;
}

static int known_cursor(acl_engine *h, acl_lookup_cursor *cur) {
    if (!h || !cur) return fail(ACL_ERR_INVALID_ARGUMENT, "lookup cursor: NULL handle");
    std::lock_guard<std::mutex> lk(h->cursors_mu);
    if (std::find(h->cursors.begin(), h->cursors.end(), cur) == h->cursors.end()) return fail(ACL_ERR_INVALID_ARGUMENT, "lookup cursor: not an open cursor of this engine");
    return ACL_OK;
}

// (caller holds cur->mu) a schema reload since the open: the ids of the rows mean nothing any more
static int cursor_live(acl_engine *h, const acl_lookup_cursor *cur) {
    std::shared_lock<std::shared_mutex> nlk(h->names_mu);
    if (h->store.schema_loads() != cur->schema_loads) return fail(ACL_ERR_FAILED_PRECONDITION, "lookup cursor: expired (the schema was reloaded since the open): reopen");
    return ACL_OK;
}

static CallOpts cursor_opts(const acl_call_opts_t *o) {
    CallOpts opts;
    if (o) {
        opts.cancel = o->cancel;
        if (o->timeout_ns > 0) opts.deadline_ns = mono_ns() + o->timeout_ns;
    }
    return opts;
}

static int cursor_open(acl_engine *h, int rtype, int perm, int stype, int srel, const uint32_t *ids, size_t n, const acl_call_opts_t *o, bool subjects,
                       acl_lookup_cursor **out) {
    if (!h || !out || (n && !ids)) return fail(ACL_ERR_INVALID_ARGUMENT, subjects ? "acl_lookup_cursor_open_subjects: NULL argument" : "acl_lookup_cursor_open: NULL argument");
    *out = nullptr;
    int key_slot = -1;
    {
        std::shared_lock<RwLock> slk(h->state_mu);
        int rc = cursor_args_ok(h, rtype, perm, stype, srel);
        if (rc) return rc;
        if (h->store_only) return fail(ACL_ERR_UNAVAILABLE, "engine was opened store-only (no GPU): lookup cursors are unavailable");
        rc = not_sharded(h);
        if (rc) return rc;
        if (srel >= 0 && !subjects) key_slot = h->store.schema().slot(stype, srel);
    }
    const CallOpts opts = cursor_opts(o);
    auto cur = std::make_unique<acl_lookup_cursor>();
    cur->rtype = rtype;
    cur->perm = perm;
    cur->stype = stype;
    cur->srel = srel;
    cur->subjects = subjects;
    {
        std::lock_guard<std::mutex> lk(h->pool_mu);  // (next_dev: where evaluations are spread from, too)
        cur->device = h->devs[h->devs.size() > 1 ? h->next_dev++ % h->devs.size() : 0]->device;
    }
    Eval ev;
    // (brings the snapshot up to date; a replica on the rows' device; the reverse rows for LookupResources' walk, the subject rows for LookupSubjects')
    int rc = ev.begin(h, !subjects, opts, key_slot, h->devs.size() > 1 ? cur->device : -1, subjects);
    if (rc) return rc;
    rc = cursor_args_ok(h, rtype, perm, stype, srel);  // (the schema may have been reloaded in between)
    if (rc == ACL_OK) rc = not_sharded(h);
    if (rc) return rc;
    PassCtx *c = ev.c;
    cur->device = c->dev->device;
    const uint32_t nobj = h->store.objects(cur->row_type()).count();
    const size_t nw = row_words_for(nobj);
    if (n > 0x7FFFFFFFull || n * nw > kCursorBytes / sizeof(uint32_t))
        return fail(ACL_ERR_RESOURCE_EXHAUSTED, "lookup cursor: the rows would exceed 1 GiB of device memory: open fewer rows per cursor");
    cur->n_rows = n;
    cur->row_words = nw;
    cur->ntiles = (uint32_t)((nw + kDiffTileWords - 1) / kDiffTileWords);
    cur->bytes = n * nw * sizeof(uint32_t);
    cur->revision = h->snap.revision;
    {
        std::shared_lock<std::shared_mutex> nlk(h->names_mu);
        cur->schema_loads = h->store.schema_loads();
        cur->ids_recycled = h->store.ids_recycled();
    }
    cur->counts.assign(n, 0);
    cur->flags.assign(n, 0);
    // the engine's budget: taken now, given back when the open fails or the cursor closes
    {
        std::lock_guard<std::mutex> lk(h->cursors_mu);
        if (h->cursor_bytes + cur->bytes > kCursorBytes)
            return fail(ACL_ERR_RESOURCE_EXHAUSTED, "lookup cursor: the open cursors of this engine would hold more than 1 GiB of rows: close some");
        h->cursor_bytes += cur->bytes;
    }
    struct Budget {
        acl_engine *h;
        size_t bytes;
        ~Budget() {
            if (!bytes) return;
            std::lock_guard<std::mutex> lk(h->cursors_mu);
            h->cursor_bytes -= bytes;
        }
    } budget{h, cur->bytes};
    HIP_TRY(hipStreamCreateWithFlags(&cur->stream, hipStreamNonBlocking));
    if (n) {
        HIP_TRY(cur->rows.ensure(n * nw));
        const uint32_t target = (uint32_t)h->store.schema().slot(rtype, perm);
        const bool nonmono = h->snap.slot_nonmono.size() > target && h->snap.slot_nonmono[target];
        if (nonmono) {
            // a permission with `&` / `-` / `.all()`: the batch call's own confirmation on host rows (lookup_refine, subjects_batch), then one upload
            std::vector<uint32_t> host(n * nw);
            rc = subjects ? subjects_batch(h, c, rtype, perm, stype, srel, ids, n, host.data(), nw, nullptr, cur->flags.data(), nullptr)
                          : lookup_batch(h, c, rtype, perm, stype, srel, ids, n, host.data(), nw, nullptr);
            if (rc) return rc;
            HIP_TRY(hipMemcpy(cur->rows.p, host.data(), n * nw * sizeof(uint32_t), hipMemcpyHostToDevice));
        } else if (subjects) {
            DevArray<uint32_t> d_flags;
            HIP_TRY(d_flags.ensure(n));
            rc = subjects_walk_device(h, c, rtype, perm, stype, srel, ids, n, SubjDevDst{cur->rows.p, nw, d_flags.p}, cur->flags.data());
            if (rc) return rc;
            for (uint8_t &f : cur->flags) f = f ? (uint8_t)ACL_SUBJECTS_WILDCARD : (uint8_t)0;
            HIP_TRY(hipStreamSynchronize(c->stream));  // (d_flags is written by the walk's last copy kernel)
        } else {
            rc = lookup_batch(h, c, rtype, perm, stype, srel, ids, n, nullptr, 0, nullptr, cur->rows.p, nw);
            if (rc) return rc;
        }
        rc = check_opts(opts);
        if (rc) return rc;
        // the rank index: per-tile counts and their exclusive scan over [row][tile] (old_nrows = 0: the old array is never read)
        const DevRowsDiff all{cur->rows.p, cur->rows.p, (uint32_t)nw, (uint32_t)nw, 0u, (uint32_t)n, nullptr};
        DevArray<uint32_t> d_counts;
        uint64_t total = 0;
        rc = rows_diff_scan(c, all, d_counts, cur->offs, 0, &total);
        if (rc) return rc;
        // the rows' counts: the index at the row boundaries (the index is 8 bytes per 16 KiB of rows: it crosses whole, in one copy)
        std::vector<uint64_t> offs(n * cur->ntiles + 1);
        HIP_TRY(hipMemcpy(offs.data(), cur->offs.p, offs.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; i++) cur->counts[i] = offs[(i + 1) * cur->ntiles] - offs[i * cur->ntiles];
    }
    {
        std::lock_guard<std::mutex> lk(h->cursors_mu);
        h->cursors.push_back(cur.get());
    }
    budget.bytes = 0;  // (the cursor's from here on)
    *out = cur.release();
    return ACL_OK;
}

// (caller holds cur->mu; the requests are validated) answers m requests: ids at ids_out + the prefix of the limits, n_out / more_out per request
static int cursor_pages(acl_engine *h, acl_lookup_cursor *cur, const acl_page_req_t *reqs, size_t m, uint64_t sum, uint32_t *ids_out, uint32_t *n_out, uint8_t *more_out) {
    HIP_TRY(hipSetDevice(cur->device));
    HIP_TRY(cur->d_reqs.ensure(m));
    HIP_TRY(cur->d_plan.ensure(m));
    HIP_TRY(cur->d_res.ensure(m));
    HIP_TRY(cur->d_ids.ensure(sum));
    HIP_TRY(cur->h_in.ensure(m * sizeof(uint4)));
    const bool one_copy = sum <= kPageOneCopyIds;
    HIP_TRY(cur->h_out.ensure((m + (one_copy ? sum : 0)) * sizeof(uint32_t)));
    uint4 *hr = (uint4 *)cur->h_in.p;
    uint32_t base = 0;
    for (size_t q = 0; q < m; q++) {  // (the reserved word travels as the request's offset into the ids)
        hr[q] = make_uint4(reqs[q].row, reqs[q].after_id, reqs[q].limit, base);
        base += reqs[q].limit;
    }
    const bool timing = h->timing.load(std::memory_order_relaxed);
    if (timing && !cur->ev[0]) {
        HIP_TRY(hipEventCreate(&cur->ev[0]));
        HIP_TRY(hipEventCreate(&cur->ev[1]));
    }
    HIP_TRY(hipMemcpyAsync(cur->d_reqs.p, hr, m * sizeof(uint4), hipMemcpyHostToDevice, cur->stream));
    if (timing) HIP_TRY(hipEventRecord(cur->ev[0], cur->stream));
    const DevRowsPage p{cur->rows.p, cur->offs.p, (uint32_t)cur->row_words, cur->ntiles, (uint32_t)cur->n_rows};
    launch_rows_page(cur->stream, p, cur->d_reqs.p, (uint32_t)m, cur->d_plan.p, cur->d_res.p, cur->d_ids.p);
    HIP_TRY(hipGetLastError());
    if (timing) HIP_TRY(hipEventRecord(cur->ev[1], cur->stream));
    uint32_t *res = (uint32_t *)cur->h_out.p, *hids = res + m;
    HIP_TRY(hipMemcpyAsync(res, cur->d_res.p, m * sizeof(uint32_t), hipMemcpyDeviceToHost, cur->stream));
    if (one_copy) HIP_TRY(hipMemcpyAsync(hids, cur->d_ids.p, sum * sizeof(uint32_t), hipMemcpyDeviceToHost, cur->stream));
    HIP_TRY(hipStreamSynchronize(cur->stream));
    float ms = 0;
    if (timing && hipEventElapsedTime(&ms, cur->ev[0], cur->ev[1]) != hipSuccess) ms = 0;
    {
        std::lock_guard<std::mutex> lk(h->stats_mu);
        h->page_launches += 2;
        h->page_ms += ms;
        h->stats.kernel_ms += ms;
    }
    if (!one_copy) {  // the written prefix of the ids: up to the end of the last request that returned any
        uint64_t hi = 0, b = 0;
        for (size_t q = 0; q < m; q++) {
            const uint32_t k = res[q] & 0x7FFFFFFFu;
            if (k) hi = b + k;
            b += reqs[q].limit;
        }
        // (res moves with a grown staging buffer: keep the counts)
        std::vector<uint32_t> keep(res, res + m);
        HIP_TRY(cur->h_out.ensure((m + hi) * sizeof(uint32_t)));
        res = (uint32_t *)cur->h_out.p;
        hids = res + m;
        std::memcpy(res, keep.data(), m * sizeof(uint32_t));
        if (hi) HIP_TRY(hipMemcpy(hids, cur->d_ids.p, hi * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    uint64_t b = 0;
    for (size_t q = 0; q < m; q++) {
        const uint32_t k = res[q] & 0x7FFFFFFFu;
        if (k) std::memcpy(ids_out + b, hids + b, k * sizeof(uint32_t));
        n_out[q] = k;
        more_out[q] = (uint8_t)(res[q] >> 31);
        b += reqs[q].limit;
    }
    return ACL_OK;
}

// the requests' own fields, before anything of the engine is looked at; *sum_out: the limits, summed
static int page_reqs_ok(const acl_page_req_t *reqs, size_t m, const uint32_t *ids_out, size_t ids_cap, uint64_t *sum_out) {
    uint64_t sum = 0;
    for (size_t q = 0; q < m; q++) {
        if (!reqs[q].limit) return fail(ACL_ERR_INVALID_ARGUMENT, "lookup cursor: request " + std::to_string(q) + ": limit is 0");
        if (reqs[q].reserved) return fail(ACL_ERR_INVALID_ARGUMENT, "lookup cursor: request " + std::to_string(q) + ": reserved is not 0");
        sum += reqs[q].limit;
        if (sum > kPageMaxIds) return fail(ACL_ERR_INVALID_ARGUMENT, "lookup cursor: the limits of one call add up to more than 2^28 ids");
    }
    if (ids_cap < sum || (sum && !ids_out)) return fail(ACL_ERR_INVALID_ARGUMENT, "lookup cursor: ids_out holds fewer ids than the limits add up to (" + std::to_string(sum) + ")");
    *sum_out = sum;
    return ACL_OK;
}

static int page_rows_ok(const acl_lookup_cursor *cur, const acl_page_req_t *reqs, size_t m) {
    for (size_t q = 0; q < m; q++)
        if (reqs[q].row >= cur->n_rows)
            return fail(ACL_ERR_INVALID_ARGUMENT, "lookup cursor: request " + std::to_string(q) + ": row " + std::to_string(reqs[q].row) + " beyond the cursor's " +
                                                      std::to_string(cur->n_rows) + " rows");
    return ACL_OK;
}

void lookup_cursors_release(acl_engine_t *h) {
    std::vector<acl_lookup_cursor *> curs;
    {
        std::lock_guard<std::mutex> lk(h->cursors_mu);
        curs.swap(h->cursors);
        h->cursor_bytes = 0;
    }
    for (acl_lookup_cursor *cur : curs) delete cur;
}

}  // namespace aclint

extern "C" {

int acl_lookup_cursor_open(acl_engine_t *h, int rtype, int permission, int stype, int srel, const uint32_t *subject_ids, size_t n, const acl_call_opts_t *opts,
                           acl_lookup_cursor_t **out) {
    return cursor_open(h, rtype, permission, stype, srel, subject_ids, n, opts, false, out);
}

int acl_lookup_cursor_open_subjects(acl_engine_t *h, int rtype, int permission, int stype, int srel, const uint32_t *resource_ids, size_t n,
                                    const acl_call_opts_t *opts, acl_lookup_cursor_t **out) {
    return cursor_open(h, rtype, permission, stype, srel, resource_ids, n, opts, true, out);
}

int acl_lookup_cursor_info(acl_engine_t *h, acl_lookup_cursor_t *cur, uint64_t *revision_out, uint32_t *n_rows_out, uint32_t *row_type_out, uint64_t *counts_out,
                           uint8_t *flags_out) {
    int rc = known_cursor(h, cur);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(cur->mu);
    rc = cursor_live(h, cur);
    if (rc) return rc;
    if (revision_out) *revision_out = cur->revision;
    if (n_rows_out) *n_rows_out = (uint32_t)cur->n_rows;
    if (row_type_out) *row_type_out = (uint32_t)cur->row_type();
    if (counts_out) std::copy(cur->counts.begin(), cur->counts.end(), counts_out);
    if (flags_out) std::copy(cur->flags.begin(), cur->flags.end(), flags_out);
    return ACL_OK;
}

int acl_lookup_cursor_pages(acl_engine_t *h, acl_lookup_cursor_t *cur, const acl_page_req_t *reqs, size_t m, uint32_t *ids_out, size_t ids_cap, uint32_t *n_out,
                            uint8_t *more_out, const acl_call_opts_t *o) {
    if (!h || !cur || (m && (!reqs || !n_out || !more_out))) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_lookup_cursor_pages: NULL argument");
    uint64_t sum = 0;
    int rc = page_reqs_ok(reqs, m, ids_out, ids_cap, &sum);
    if (rc) return rc;
    rc = known_cursor(h, cur);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(cur->mu);
    rc = page_rows_ok(cur, reqs, m);
    if (rc == ACL_OK) rc = cursor_live(h, cur);
    if (rc == ACL_OK) rc = check_opts(cursor_opts(o));
    if (rc || !m) return rc;
    return cursor_pages(h, cur, reqs, m, sum, ids_out, n_out, more_out);
}

int acl_lookup_cursor_page_names(acl_engine_t *h, acl_lookup_cursor_t *cur, uint32_t row, uint32_t after_id, uint32_t limit, uint32_t *ids_out, char *buf, size_t cap,
                                 uint32_t *ends, uint32_t *n_out, uint8_t *more_out) {
    if (!h || !cur || !ids_out || !buf || !ends || !n_out || !more_out || cap < 1024 || cap > 0xFFFFFFFFull)
        return fail(ACL_ERR_INVALID_ARGUMENT, "acl_lookup_cursor_page_names: bad argument (buf must hold at least 1024 bytes: the longest object id)");
    const acl_page_req_t rq{row, after_id, limit, 0u};
    uint64_t sum = 0;
    int rc = page_reqs_ok(&rq, 1, ids_out, limit, &sum);
    if (rc) return rc;
    rc = known_cursor(h, cur);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(cur->mu);
    rc = page_rows_ok(cur, &rq, 1);
    if (rc == ACL_OK) rc = cursor_live(h, cur);
    if (rc) return rc;
    uint32_t k = 0;
    uint8_t more = 0;
    rc = cursor_pages(h, cur, &rq, 1, sum, ids_out, &k, &more);  // (a refusal below leaves the page's ids in ids_out: they are right, only unnamed)
    if (rc) return rc;
    std::shared_lock<std::shared_mutex> nlk(h->names_mu);  // (held over the check AND the names: no id changes its name in between)
    if (h->store.schema_loads() != cur->schema_loads || h->store.ids_recycled() != cur->ids_recycled)
        return fail(ACL_ERR_FAILED_PRECONDITION, "lookup cursor: expired for names (an object id was recycled since the open): reopen");
    const ObjectTable &ot = h->store.objects(cur->row_type());
    size_t used = 0;
    uint32_t got = 0;
    for (; got < k; got++) {
        const std::string *nm = ot.name(ids_out[got]);  // (an anonymous bulk-loaded id: an empty name, as acl_bitmap_names)
        const size_t len = nm ? nm->size() : 0;
        if (used + len > cap) break;  // (the caller continues behind the last id returned: cap >= the longest id, so a call always makes progress)
        if (len) std::memcpy(buf + used, nm->data(), len);
        used += len;
        ends[got] = (uint32_t)used;
    }
    *n_out = got;
    *more_out = (uint8_t)((more || got < k) ? 1 : 0);
    return ACL_OK;
}

int acl_lookup_cursor_close(acl_engine_t *h, acl_lookup_cursor_t *cur) {
    if (!h || !cur) return fail(ACL_ERR_INVALID_ARGUMENT, "lookup cursor: NULL handle");
    {
        std::lock_guard<std::mutex> lk(h->cursors_mu);
        auto it = std::find(h->cursors.begin(), h->cursors.end(), cur);
        if (it == h->cursors.end()) return fail(ACL_ERR_INVALID_ARGUMENT, "lookup cursor: not an open cursor of this engine");
        h->cursors.erase(it);
        h->cursor_bytes -= cur->bytes;
    }
    { std::lock_guard<std::mutex> lk(cur->mu); }  // (a page in flight finishes first; no call on a cursor may be started after its close)
    delete cur;
    return ACL_OK;
}

int acl_lookup_cursor_stats(acl_engine_t *h, uint64_t *page_launches_out, double *page_ms_out) {
    if (!h) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_lookup_cursor_stats: NULL handle");
    std::lock_guard<std::mutex> lk(h->stats_mu);
    if (page_launches_out) *page_launches_out = h->page_launches;
    if (page_ms_out) *page_ms_out = h->page_ms;
    return ACL_OK;
}

}  // extern "C"

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
// A mixed open is the same open with one walk per run of subjects of one form, all inside the one evaluation.  A derive takes no snapshot and no
// context either: its operands are rows of open cursors, held by their mutexes (locked in address order), and its result is a new cursor's rows (or, for a
// count, nothing but the counts) -- two launches (kernels.hip k_rows_derive, then the diff's scan), on the new cursor's stream.
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

// What an open and a derive share around the making of the rows.  reserve: the cursor's shape, its share of the engine's budget (given back by the guard unless
// the cursor is published), its stream and its rows.  counts_from_index: the rows' counts are the rank index at the row boundaries (the index is 8 bytes per
// 16 KiB of rows: it crosses whole, in one copy on the cursor's own stream).  publish: the cursor becomes one of the engine's open cursors.
struct CursorBudget {
    acl_engine *h = nullptr;
    size_t bytes = 0;
    ~CursorBudget() {
        if (!bytes) return;
        std::lock_guard<std::mutex> lk(h->cursors_mu);
        h->cursor_bytes -= bytes;
    }
};

static int cursor_reserve(acl_engine *h, acl_lookup_cursor *cur, size_t n, size_t nw, CursorBudget *budget) {
    if (n > 0x7FFFFFFFull || n * nw > kCursorBytes / sizeof(uint32_t))
        return fail(ACL_ERR_RESOURCE_EXHAUSTED, "lookup cursor: the rows would exceed 1 GiB of device memory: open fewer rows per cursor");
    cur->n_rows = n;
    cur->row_words = nw;
    cur->ntiles = (uint32_t)((nw + kDiffTileWords - 1) / kDiffTileWords);
    cur->bytes = n * nw * sizeof(uint32_t);
    cur->counts.assign(n, 0);
    cur->flags.assign(n, 0);
    {
        std::lock_guard<std::mutex> lk(h->cursors_mu);
        if (h->cursor_bytes + cur->bytes > kCursorBytes)
            return fail(ACL_ERR_RESOURCE_EXHAUSTED, "lookup cursor: the open cursors of this engine would hold more than 1 GiB of rows: close some");
        h->cursor_bytes += cur->bytes;
    }
    budget->h = h;
    budget->bytes = cur->bytes;
    HIP_TRY(hipStreamCreateWithFlags(&cur->stream, hipStreamNonBlocking));
    if (n) HIP_TRY(cur->rows.ensure(n * nw));
    return ACL_OK;
}

// counts[i] = offs[(i + 1) * ntiles] - offs[i * ntiles] of a rank index on the device (written on `st`, which is synchronised here)
static int counts_from_index(hipStream_t st, const uint64_t *d_offs, size_t n, uint32_t ntiles, uint64_t *counts) {
    std::vector<uint64_t> offs(n * ntiles + 1);
    HIP_TRY(hipMemcpyAsync(offs.data(), d_offs, offs.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t i = 0; i < n; i++) counts[i] = offs[(i + 1) * ntiles] - offs[i * ntiles];
    return ACL_OK;
}

static void cursor_publish(acl_engine *h, std::unique_ptr<acl_lookup_cursor> &cur, CursorBudget *budget, acl_lookup_cursor **out) {
    {
        std::lock_guard<std::mutex> lk(h->cursors_mu);
        h->cursors.push_back(cur.get());
    }
    budget->bytes = 0;  // (the cursor's from here on)
    *out = cur.release();
}

// consecutive rows [first, first + count) of an open whose subjects (resources, for a subject cursor) share one (stype, srel): one walk each
struct CursorRun {
    int stype, srel;
    size_t first, count;
};

static int cursor_open(acl_engine *h, int rtype, int perm, const std::vector<CursorRun> &runs, const uint32_t *ids, size_t n, const acl_call_opts_t *o, bool subjects,
                       acl_lookup_cursor **out) {
    *out = nullptr;
    std::vector<int> key_slots;
    const auto runs_ok = [&]() {
        for (const CursorRun &r : runs)
            if (int rc = cursor_args_ok(h, rtype, perm, r.stype, r.srel)) return rc;
        return (int)ACL_OK;
    };
    {
        std::shared_lock<RwLock> slk(h->state_mu);
        int rc = runs_ok();
        if (rc) return rc;
        if (h->store_only) return fail(ACL_ERR_UNAVAILABLE, "engine was opened store-only (no GPU): lookup cursors are unavailable");
        rc = not_sharded(h);
        if (rc) return rc;
        for (const CursorRun &r : runs)
            if (r.srel >= 0 && !subjects) key_slots.push_back(h->store.schema().slot(r.stype, r.srel));
    }
    const CallOpts opts = call_opts(o);
    auto cur = std::make_unique<acl_lookup_cursor>();
    cur->rtype = rtype;
    cur->perm = perm;
    cur->stype = runs[0].stype;  // (what a subject cursor's rows are ids of; a mixed open has no single subject form and does not need one)
    cur->srel = runs[0].srel;
    cur->subjects = subjects;
    {
        std::lock_guard<std::mutex> lk(h->pool_mu);  // (next_dev: where evaluations are spread from, too)
        cur->device = h->devs[h->devs.size() > 1 ? h->next_dev++ % h->devs.size() : 0]->device;
    }
    Eval ev;
    // (brings the snapshot up to date; a replica on the rows' device; the reverse rows for LookupResources' walk, the subject rows for LookupSubjects')
    int rc = ev.begin(h, !subjects, opts, -1, h->devs.size() > 1 ? cur->device : -1, subjects, &key_slots);
    if (rc) return rc;
    rc = runs_ok();  // (the schema may have been reloaded in between)
    if (rc == ACL_OK) rc = not_sharded(h);
    if (rc) return rc;
    PassCtx *c = ev.c;
    cur->device = c->dev->device;
    const uint32_t nobj = h->store.objects(cur->row_type()).count();
    const size_t nw = row_words_for(nobj);
    cur->revision = h->snap.revision;
    {
        std::shared_lock<std::shared_mutex> nlk(h->names_mu);
        cur->schema_loads = h->store.schema_loads();
        cur->ids_recycled = h->store.ids_recycled();
    }
    // the engine's budget: taken now, given back when the open fails or the cursor closes
    CursorBudget budget;
    rc = cursor_reserve(h, cur.get(), n, nw, &budget);
    if (rc) return rc;
    if (n) {
        const uint32_t target = (uint32_t)h->store.schema().slot(rtype, perm);
        const bool nonmono = h->snap.slot_nonmono.size() > target && h->snap.slot_nonmono[target];
        for (const CursorRun &r : runs) {
            if (!r.count) continue;
            const uint32_t *rids = ids + r.first;
            uint32_t *d_rows = cur->rows.p + r.first * nw;
            if (nonmono) {
                // a permission with `&` / `-` / `.all()`: the batch call's own confirmation on host rows (lookup_refine, subjects_batch), then one upload
                std::vector<uint32_t> host(r.count * nw);
                rc = subjects ? subjects_batch(h, c, rtype, perm, r.stype, r.srel, rids, r.count, host.data(), nw, nullptr, cur->flags.data() + r.first, nullptr)
                              : lookup_batch(h, c, rtype, perm, r.stype, r.srel, rids, r.count, host.data(), nw, nullptr);
                if (rc) return rc;
                HIP_TRY(hipMemcpy(d_rows, host.data(), r.count * nw * sizeof(uint32_t), hipMemcpyHostToDevice));
            } else if (subjects) {
                DevArray<uint32_t> d_flags;
                HIP_TRY(d_flags.ensure(r.count));
                rc = subjects_walk_device(h, c, rtype, perm, r.stype, r.srel, rids, r.count, SubjDevDst{d_rows, nw, d_flags.p}, cur->flags.data() + r.first);
                if (rc) return rc;
                for (size_t i = r.first; i < r.first + r.count; i++) cur->flags[i] = cur->flags[i] ? (uint8_t)ACL_SUBJECTS_WILDCARD : (uint8_t)0;
                HIP_TRY(hipStreamSynchronize(c->stream));  // (d_flags is written by the walk's last copy kernel)
            } else {
                rc = lookup_batch(h, c, rtype, perm, r.stype, r.srel, rids, r.count, nullptr, 0, nullptr, d_rows, nw);
                if (rc) return rc;
            }
        }
        rc = check_opts(opts);
        if (rc) return rc;
        // the rank index: per-tile counts and their exclusive scan over [row][tile] (old_nrows = 0: the old array is never read)
        const DevRowsDiff all{cur->rows.p, cur->rows.p, (uint32_t)nw, (uint32_t)nw, 0u, (uint32_t)n, nullptr};
        DevArray<uint32_t> d_counts;
        uint64_t total = 0;
        rc = rows_diff_scan(c, all, d_counts, cur->offs, 0, &total);  // (synchronises c's stream: the rows and the index are there)
        if (rc) return rc;
        rc = counts_from_index(cur->stream, cur->offs.p, n, cur->ntiles, cur->counts.data());
        if (rc) return rc;
    }
    cursor_publish(h, cur, &budget, out);
    return ACL_OK;
}

static int cursor_open_one(acl_engine *h, int rtype, int perm, int stype, int srel, const uint32_t *ids, size_t n, const acl_call_opts_t *o, bool subjects,
                           acl_lookup_cursor **out) {
    if (!h || !out || (n && !ids)) return fail(ACL_ERR_INVALID_ARGUMENT, subjects ? "acl_lookup_cursor_open_subjects: NULL argument" : "acl_lookup_cursor_open: NULL argument");
    return cursor_open(h, rtype, perm, {CursorRun{stype, srel, 0, n}}, ids, n, o, subjects, out);
}

// ---- derived cursors ----
// The sources of one derive / count call: validated, locked in address order (a cursor named twice is locked once), and what the rules ask of them.
struct DeriveSources {
    std::vector<acl_lookup_cursor *> srcs;
    std::vector<std::unique_lock<std::mutex>> locks;
    const acl_lookup_cursor *first() const { return srcs.empty() ? nullptr : srcs[0]; }
};

// the call's own fields, before any cursor or anything of the engine is looked at
static int derive_fields_ok(size_t n_srcs, const acl_row_ref_t *refs, size_t n_refs, const acl_row_expr_t *exprs, size_t n_exprs, uint32_t flags) {
    if (flags & ~ACL_DERIVE_ANY_REVISION) return fail(ACL_ERR_INVALID_ARGUMENT, "lookup derive: unknown flag bits");
    if (n_srcs > 0xFFFFFFFFull || n_refs > 0x7FFFFFFFull || n_exprs > 0x7FFFFFFFull) return fail(ACL_ERR_INVALID_ARGUMENT, "lookup derive: more than 2^31 sources, refs or expressions");
    for (size_t k = 0; k < n_refs; k++)
        if (refs[k].cursor >= n_srcs)
            return fail(ACL_ERR_INVALID_ARGUMENT, "lookup derive: ref " + std::to_string(k) + ": cursor " + std::to_string(refs[k].cursor) + " beyond the " + std::to_string(n_srcs) + " sources");
    for (size_t e = 0; e < n_exprs; e++) {
        const acl_row_expr_t &x = exprs[e];
        if ((uint64_t)x.first + x.n_any + x.n_all + x.n_none > n_refs)
            return fail(ACL_ERR_INVALID_ARGUMENT, "lookup derive: expression " + std::to_string(e) + " runs past the " + std::to_string(n_refs) + " refs");
        if ((uint64_t)x.n_any + x.n_all == 0)
            return fail(ACL_ERR_INVALID_ARGUMENT, "lookup derive: expression " + std::to_string(e) + ": n_any + n_all is 0 (\"everything\" is never materialised)");
    }
    return ACL_OK;
}

// one evaluation of the expressions on the sources' device.  out != NULL: a new cursor keeps the rows; else counts_out gets the rows' counts and nothing is kept.
static int cursor_derive(acl_engine *h, acl_lookup_cursor *const *srcs_in, size_t n_srcs, const acl_row_ref_t *refs, size_t n_refs, const acl_row_expr_t *exprs,
                         size_t n_exprs, uint32_t flags, acl_lookup_cursor **out, uint64_t *counts_out, const char *fn) {
    if (!h || (n_srcs && !srcs_in) || (n_refs && !refs) || (n_exprs && !exprs)) return fail(ACL_ERR_INVALID_ARGUMENT, std::string(fn) + ": NULL argument");
    for (size_t i = 0; i < n_srcs; i++)
        if (!srcs_in[i]) return fail(ACL_ERR_INVALID_ARGUMENT, std::string(fn) + ": NULL argument (source " + std::to_string(i) + ")");
    int rc = derive_fields_ok(n_srcs, refs, n_refs, exprs, n_exprs, flags);
    if (rc) return rc;
    DeriveSources S;
    S.srcs.assign(srcs_in, srcs_in + n_srcs);
    for (acl_lookup_cursor *s : S.srcs)
        if ((rc = known_cursor(h, s))) return rc;
    {
        std::vector<acl_lookup_cursor *> order(S.srcs);
        std::sort(order.begin(), order.end(), std::less<acl_lookup_cursor *>());
        order.erase(std::unique(order.begin(), order.end()), order.end());
        for (acl_lookup_cursor *s : order) S.locks.emplace_back(s->mu);
    }
    for (size_t k = 0; k < n_refs; k++)
        if (refs[k].row >= S.srcs[refs[k].cursor]->n_rows)
            return fail(ACL_ERR_INVALID_ARGUMENT, "lookup derive: ref " + std::to_string(k) + ": row " + std::to_string(refs[k].row) + " beyond the source's " +
                                                      std::to_string(S.srcs[refs[k].cursor]->n_rows) + " rows");
    const acl_lookup_cursor *s0 = S.first();
    for (const acl_lookup_cursor *s : S.srcs)
        if (s->subjects != s0->subjects || s->row_type() != s0->row_type())
            return fail(ACL_ERR_INVALID_ARGUMENT, "lookup derive: the sources differ in direction or in the type of their rows' ids");
    {
        std::shared_lock<RwLock> slk(h->state_mu);
        if (h->store_only) return fail(ACL_ERR_UNAVAILABLE, "engine was opened store-only (no GPU): lookup cursors are unavailable");
        rc = not_sharded(h);
        if (rc) return rc;
    }
    // the preconditions: live, one revision (or the smallest), one device, no wildcard row under an expression
    uint64_t revision = s0 ? s0->revision : 0, ids_recycled = s0 ? s0->ids_recycled : 0;
    size_t nw = 4;
    for (const acl_lookup_cursor *s : S.srcs) {
        if ((rc = cursor_live(h, s))) return rc;
        if (s->revision != revision && !(flags & ACL_DERIVE_ANY_REVISION))
            return fail(ACL_ERR_FAILED_PRECONDITION, "lookup derive: the sources were opened at different revisions (ACL_DERIVE_ANY_REVISION allows it)");
        if (s->device != s0->device) return fail(ACL_ERR_FAILED_PRECONDITION, "lookup derive: the sources' rows live on different devices");
        revision = std::min(revision, s->revision);
        ids_recycled = std::min(ids_recycled, s->ids_recycled);
        nw = std::max(nw, s->row_words);
    }
    for (size_t e = 0; e < n_exprs; e++)
        for (size_t k = exprs[e].first, end = k + exprs[e].n_any + exprs[e].n_all + exprs[e].n_none; k < end; k++) {
            const acl_lookup_cursor *s = S.srcs[refs[k].cursor];
            if (s->subjects && (s->flags[refs[k].row] & ACL_SUBJECTS_WILDCARD))
                return fail(ACL_ERR_FAILED_PRECONDITION, "lookup derive: expression " + std::to_string(e) + " references row " + std::to_string(refs[k].row) +
                                                             " of source " + std::to_string(refs[k].cursor) + ", which holds a wildcard (\"everyone but ...\" is not a bitmap)");
        }
    std::unique_ptr<acl_lookup_cursor> cur;
    CursorBudget budget;
    uint64_t schema_loads = s0 ? s0->schema_loads : 0;
    int device = s0 ? s0->device : 0;
    if (!s0) {  // (no sources, so no expressions: a cursor without rows, marked as an open at this moment would be)
        std::shared_lock<RwLock> slk(h->state_mu);
        std::shared_lock<std::shared_mutex> nlk(h->names_mu);
        device = h->devs[0]->device;
        schema_loads = h->store.schema_loads();
        ids_recycled = h->store.ids_recycled();
    }
    HIP_TRY(hipSetDevice(device));
    const uint32_t ntiles = (uint32_t)((nw + kDiffTileWords - 1) / kDiffTileWords);
    if (out) {
        cur = std::make_unique<acl_lookup_cursor>();
        if (s0) {
            cur->rtype = s0->rtype, cur->perm = s0->perm, cur->stype = s0->stype, cur->srel = s0->srel;
            cur->subjects = s0->subjects;
        }
        cur->device = device;
        cur->revision = revision;
        cur->schema_loads = schema_loads;
        cur->ids_recycled = ids_recycled;
        rc = cursor_reserve(h, cur.get(), n_exprs, nw, &budget);
        if (rc) return rc;
    }
    if (n_exprs) {
        // the operand records {row base, words}; the expression records travel as they are
        std::vector<ulonglong2> ops(n_refs);
        for (size_t k = 0; k < n_refs; k++) {
            const acl_lookup_cursor *s = S.srcs[refs[k].cursor];
            ops[k] = make_ulonglong2((unsigned long long)(uintptr_t)(s->rows.p + (size_t)refs[k].row * s->row_words), (unsigned long long)s->row_words);
        }
        static_assert(sizeof(acl_row_expr_t) == sizeof(uint4) && sizeof(ulonglong2) == 16, "the kernel's 16-byte records");
        // (a count runs on the first source's stream, whose mutex this call holds: n_exprs > 0 means there is a source)
        hipStream_t st = cur ? cur->stream : s0->stream;
        // one scratch allocation of 16-byte units: the expression records, the operand records, the tile counts and, for a count, the index
        const size_t tiles = n_exprs * ntiles, u_ops = n_exprs, u_counts = u_ops + std::max<size_t>(n_refs, 1), u_offs = u_counts + (tiles + 3) / 4;
        DevArray<uint4> scratch;
        HIP_TRY(scratch.ensure(u_offs + (cur ? 0 : (tiles + 1 + 1) / 2)));
        uint4 *d_exprs = scratch.p;
        ulonglong2 *d_ops = reinterpret_cast<ulonglong2 *>(scratch.p + u_ops);
        uint32_t *d_counts = reinterpret_cast<uint32_t *>(scratch.p + u_counts);
        if (cur) HIP_TRY(cur->offs.ensure(tiles + 1));
        uint64_t *d_offs = cur ? cur->offs.p : reinterpret_cast<uint64_t *>(scratch.p + u_offs);
        HIP_TRY(hipMemcpyAsync(d_exprs, exprs, n_exprs * sizeof(uint4), hipMemcpyHostToDevice, st));
        if (n_refs) HIP_TRY(hipMemcpyAsync(d_ops, ops.data(), n_refs * sizeof(ulonglong2), hipMemcpyHostToDevice, st));
        const bool timing = h->timing.load(std::memory_order_relaxed);
        hipEvent_t evs[2] = {nullptr, nullptr};
        struct EvGuard {
            hipEvent_t *e;
            ~EvGuard() {
                for (int i = 0; i < 2; i++)
                    if (e[i]) (void)hipEventDestroy(e[i]);
            }
        } evg{evs};
        if (timing) {
            HIP_TRY(hipEventCreate(&evs[0]));
            HIP_TRY(hipEventCreate(&evs[1]));
            HIP_TRY(hipEventRecord(evs[0], st));
        }
        const DevRowsDerive d{d_exprs, d_ops, cur ? cur->rows.p : nullptr, (uint32_t)nw, ntiles, (uint32_t)n_exprs};
        launch_rows_derive(st, d, d_counts, d_offs);
        HIP_TRY(hipGetLastError());
        if (timing) HIP_TRY(hipEventRecord(evs[1], st));
        rc = counts_from_index(st, d_offs, n_exprs, ntiles, cur ? cur->counts.data() : counts_out);
        if (rc) return rc;
        float ms = 0;
        if (timing && hipEventElapsedTime(&ms, evs[0], evs[1]) != hipSuccess) ms = 0;
        std::lock_guard<std::mutex> lk(h->stats_mu);
        h->derive_launches += 2;
        h->derive_ms += ms;
        h->stats.kernel_ms += ms;
    }
    if (out) cursor_publish(h, cur, &budget, out);
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
    return cursor_open_one(h, rtype, permission, stype, srel, subject_ids, n, opts, false, out);
}

int acl_lookup_cursor_open_subjects(acl_engine_t *h, int rtype, int permission, int stype, int srel, const uint32_t *resource_ids, size_t n,
                                    const acl_call_opts_t *opts, acl_lookup_cursor_t **out) {
    return cursor_open_one(h, rtype, permission, stype, srel, resource_ids, n, opts, true, out);
}

int acl_lookup_cursor_open_mixed(acl_engine_t *h, int rtype, int permission, const acl_subject_ref_t *subjects, size_t n, const acl_call_opts_t *opts,
                                 acl_lookup_cursor_t **out) {
    if (!h || !out || (n && !subjects)) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_lookup_cursor_open_mixed: NULL argument");
    *out = nullptr;
    std::vector<uint32_t> ids(n);
    std::vector<CursorRun> runs;
    for (size_t i = 0; i < n; i++) {
        if (subjects[i].reserved) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_lookup_cursor_open_mixed: subject " + std::to_string(i) + ": reserved is not 0");
        ids[i] = subjects[i].id;
        if (runs.empty() || runs.back().stype != subjects[i].stype || runs.back().srel != subjects[i].srel) runs.push_back(CursorRun{subjects[i].stype, subjects[i].srel, i, 0});
        runs.back().count++;
    }
    if (runs.empty()) runs.push_back(CursorRun{rtype, -1, 0, 0});  // (no subject names a form: the type and the permission are still checked)
    return cursor_open(h, rtype, permission, runs, ids.data(), n, opts, false, out);
}

int acl_lookup_cursor_derive(acl_engine_t *h, acl_lookup_cursor_t *const *srcs, size_t n_srcs, const acl_row_ref_t *refs, size_t n_refs, const acl_row_expr_t *exprs,
                             size_t n_exprs, uint32_t flags, acl_lookup_cursor_t **out) {
    if (!out) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_lookup_cursor_derive: NULL argument");
    *out = nullptr;
    return cursor_derive(h, srcs, n_srcs, refs, n_refs, exprs, n_exprs, flags, out, nullptr, "acl_lookup_cursor_derive");
}

int acl_lookup_cursor_count(acl_engine_t *h, acl_lookup_cursor_t *const *srcs, size_t n_srcs, const acl_row_ref_t *refs, size_t n_refs, const acl_row_expr_t *exprs,
                            size_t n_exprs, uint32_t flags, uint64_t *counts_out) {
    if (n_exprs && !counts_out) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_lookup_cursor_count: NULL argument");
    return cursor_derive(h, srcs, n_srcs, refs, n_refs, exprs, n_exprs, flags, nullptr, counts_out, "acl_lookup_cursor_count");
}

int acl_lookup_derive_stats(acl_engine_t *h, uint64_t *derive_launches_out, double *derive_ms_out) {
    if (!h) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_lookup_derive_stats: NULL handle");
    std::lock_guard<std::mutex> lk(h->stats_mu);
    if (derive_launches_out) *derive_launches_out = h->derive_launches;
    if (derive_ms_out) *derive_ms_out = h->derive_ms;
    return ACL_OK;
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
    if (rc == ACL_OK) rc = check_opts(call_opts(o));
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

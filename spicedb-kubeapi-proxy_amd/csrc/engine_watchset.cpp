// engine_watchset.cpp -- watch sets (include/aclgpu.h "watch sets"): the LookupResources rows of many watchers of one
// (type, permission) kept in device memory between polls, and the poll that walks them all on the current snapshot, XORs new against old rows on the
// device (kernels.hip k_rows_diff_*) and brings back only the changes.
//
// The reference's RunWatch (pkg/authz/watch.go:27-111) hears updates of the watched type only (watch.go:29-31) and re-checks the updated object
// (watch.go:50-67); what it cannot hear -- a membership, a nesting, a namespace grant, an expiry -- is exactly what this file reports.
//
// State of a set: two device row arrays, `old` (the baseline: the rows of the last successful poll, [old_nrows][old_words]) and `new` (scratch between
// polls, [watchers][words of the snapshot at hand]).  A poll writes `new`, diffs, and only when everything succeeded swaps the two: a failed poll leaves
// the baseline alone.  Rows are dense and ordered by watcher id (ids count up, adds append, a removal closes the gap), so the diff's (row, bit) order is
// the answer's (watcher, resource id) order.  Watchers added since the last poll have no old row: the diff reads rows >= old_nrows as empty.
// A SUBJECT-direction set (acl_watch_set_open_subjects) turns the question round: its watchers are resources of the type, its rows their
// LookupSubjects answers, bits are subject ids.  The rows are walked by k_subj_local into the fresh array, a permission with `&` / `-` / `.all()` has its
// candidates confirmed where they are (subject_rows below), and the same diff and swap follow.
// Locking: the set's mutex for the whole poll (polls of one set serialise), then an ordinary evaluation (state_mu shared + a context of the pool).
#include "engine_internal.hpp"
#include "validate.hpp"

namespace aclint {
// scratch of the subject direction's device path (a set's own, or a selfcheck call's)
struct SubjScratch {
    DevArray<uint32_t> d_rids, d_flags, d_wrows, d_counts, d_status;
    DevArray<uint64_t> d_offs;
    DevArray<uint4> d_recs;
};
}  // namespace aclint

struct acl_watch_set {
    std::mutex mu;
    int rtype = 0, perm = 0, stype = 0, srel = -1;
    bool subjects = false;  // direction: the watchers are resources of rtype and the rows hold subject ids of stype (acl_watch_set_open_subjects)
    int watched_type() const { return subjects ? rtype : stype; }  // the type of the ids in `sids`
    int row_type() const { return subjects ? stype : rtype; }      // the type of the ids the rows' bits (and the records) name
    SubjScratch subj;
    int device = 0;  // HIP ordinal the rows live on
    // per row, ascending by watcher id; sids: the watched objects' ids (subjects; resources in a subject-direction set)
    std::vector<uint32_t> ids, sids;
    std::vector<uint8_t> from_now;  // 1: added with ACL_WATCHER_FROM_NOW and not polled yet -- its first diff is suppressed
    uint32_t next_id = 0;
    DevArray<uint32_t> rows[2];
    int cur = 0;  // rows[cur]: old, rows[cur ^ 1]: new
    size_t old_words = 0, old_need = 0, old_nrows = 0;  // old_need: the words the type's ids needed then (old_words: rounded up to 4)
    bool polled = false, dirty = false;  // dirty: a watcher was added since the last successful poll
    uint64_t epoch = 0, revision = 0;    // acl_engine::snap_epoch / Snapshot::revision of the last successful poll
    // the diff's scratch
    DevArray<uint32_t> d_ids, d_counts;
    DevArray<uint64_t> d_offs;
    DevArray<uint4> d_recs;
    uint64_t polls = 0, walks = 0, changes = 0;
};

namespace aclint {

constexpr size_t kWatchSetBytes = (size_t)1 << 30;     // both row arrays of a set, at most (the bound lookup_batch puts on a group's visited bits)
constexpr uint64_t kWatchSetMaxChanges = 1ull << 28;  // records of one poll, at most (4 GiB)

static int set_args_ok(acl_engine *h, int rtype, int perm, int stype, int srel) {
    if (!h->store.has_schema()) return fail(ACL_ERR_FAILED_PRECONDITION, "no schema loaded");
    const Schema &sc = h->store.schema();
    if (rtype < 0 || rtype >= (int)sc.defs.size() || stype < 0 || stype >= (int)sc.defs.size() || perm < 0 || perm >= (int)sc.defs[rtype].members.size() || srel < -1 ||
        srel >= (int)sc.defs[stype].members.size())
        return fail(ACL_ERR_FAILED_PRECONDITION, "watch set: unknown type, permission or subject relation");
    return ACL_OK;
}

// count + scan on c's stream; the total crosses once.  The tile offsets stay in d_offs ([tiles + 1], the last one the total).
int rows_diff_scan(PassCtx *c, const DevRowsDiff &d, DevArray<uint32_t> &d_counts, DevArray<uint64_t> &d_offs, int kind, uint64_t *total_out) {
    const uint64_t tiles = (uint64_t)rows_diff_tiles(d) * d.n_rows;
    HIP_TRY(d_counts.ensure(tiles));
    HIP_TRY(d_offs.ensure(tiles + 1));
    HIP_TRY(c->h_out.ensure(64));
    ev_begin(c, kind);
    launch_rows_diff_count(c->stream, d, d_counts.p, d_offs.p);
    ev_end(c);
    HIP_TRY(hipMemcpyAsync(c->h_out.p, d_offs.p + tiles, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *total_out = *(const uint64_t *)c->h_out.p;
    ev_collect(c);
    return ACL_OK;
}

// the `total` records of a scanned diff into d_recs, left on the device (enqueued only)
static int rows_diff_emit(PassCtx *c, const DevRowsDiff &d, const DevArray<uint64_t> &d_offs, DevArray<uint4> &d_recs, int kind, uint64_t total) {
    static_assert(sizeof(acl_watch_change_t) == sizeof(uint4), "a record is one 16-byte store");
    HIP_TRY(d_recs.ensure(total));
    ev_begin(c, kind);
    launch_rows_diff_emit(c->stream, d, d_offs.p, d_recs.p, total);
    ev_end(c);
    return ACL_OK;
}

// count + scan + emit on c's stream; *out (malloc) holds *n_out records afterwards.  The total crosses once, the records in one copy.
static int rows_diff(PassCtx *c, const DevRowsDiff &d, DevArray<uint32_t> &d_counts, DevArray<uint64_t> &d_offs, DevArray<uint4> &d_recs, acl_watch_change_t **out,
                     size_t *n_out) {
    uint64_t total = 0;
    *out = nullptr;
    *n_out = 0;
    int rc = rows_diff_scan(c, d, d_counts, d_offs, 0, &total);
    if (rc) return rc;
    if (!total) return ACL_OK;
    if (total > kWatchSetMaxChanges) return fail(ACL_ERR_RESOURCE_EXHAUSTED, "watch set: more than 2^28 changes in one poll (" + std::to_string(total) + ")");
    HIP_TRY(d_recs.ensure(total));
    auto *host = (acl_watch_change_t *)std::malloc(total * sizeof(acl_watch_change_t));
    if (!host) return fail(ACL_ERR_RESOURCE_EXHAUSTED, "out of host memory for the watch set's changes");
    rc = rows_diff_emit(c, d, d_offs, d_recs, 0, total);
    if (rc) {
        std::free(host);
        return rc;
    }
    hipError_t e = hipMemcpyAsync(host, d_recs.p, total * sizeof(acl_watch_change_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        std::free(host);
        return fail(ACL_ERR_INTERNAL, std::string("watch set: copy of the changes: ") + hipGetErrorString(e));
    }
    ev_collect(c);
    *out = host;
    *n_out = (size_t)total;
    return ACL_OK;
}

// The rows a subject-direction set holds for resources rids[0 .. W) on the snapshot at hand, into d_rows ([W][nw], device): after it, bit s of row i is set
// iff acl_lookup_subjects_batch reports s for rids[i]; where its answer carries ACL_SUBJECTS_WILDCARD the wildcard object's bit is set as well, and on a
// permission with `&` / `-` / `.all()` such a row holds every id of the type that holds the permission (include/aclgpu.h).  Nothing but a few bytes per row
// crosses PCIe: the walk's flags, the candidates' tile offsets, one status word per slice.  Enqueued on c's stream; not synchronised at the end.
// Caller holds an Eval with the subject rows current.
static int subject_rows(acl_engine *h, PassCtx *c, int rt, int pm, int st, int srel, const uint32_t *rids, size_t W, uint32_t *d_rows, size_t nw, SubjScratch &x) {
    if (!W) return ACL_OK;
    const uint32_t nobj = h->store.objects(st).count(), need = (uint32_t)(((size_t)nobj + 31) / 32), wid = h->store.wildcard_id(st);
    if (W > 0x7FFFFFFFull || W * nw >= ((size_t)1 << 28) + 4) return fail(ACL_ERR_RESOURCE_EXHAUSTED, "subject rows: more than 1 GiB of rows");
    HIP_TRY(x.d_flags.ensure(W));
    HIP_TRY(x.d_rids.ensure(W));
    std::vector<uint8_t> wild(W, 0);
    int rc = subjects_walk_device(h, c, rt, pm, st, srel, rids, W, SubjDevDst{d_rows, nw, x.d_flags.p}, wild.data());
    if (rc) return rc;
    std::vector<uint32_t> wrows;  // the rows whose walk reached `T:*`, ascending
    for (size_t i = 0; i < W; i++)
        if (wild[i]) wrows.push_back((uint32_t)i);
    const uint32_t target = (uint32_t)h->store.schema().slot(rt, pm);
    const bool nonmono = h->snap.slot_nonmono.size() > target && h->snap.slot_nonmono[target];
    if (nonmono) {
        // (h_in: the walk is done with it; the stream is idle behind the walk's last synchronisation, so the staging is not read while it is rewritten)
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(c->h_in.ensure((W + wrows.size()) * sizeof(uint32_t)));
        std::memcpy(c->h_in.p, rids, W * sizeof(uint32_t));
        HIP_TRY(hipMemcpyAsync(x.d_rids.p, c->h_in.p, W * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(x.d_wrows.ensure(wrows.size()));
        if (!wrows.empty()) {
            std::memcpy((uint32_t *)c->h_in.p + W, wrows.data(), wrows.size() * sizeof(uint32_t));
            HIP_TRY(hipMemcpyAsync(x.d_wrows.p, (uint32_t *)c->h_in.p + W, wrows.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        }
        HIP_TRY(x.d_status.ensure(1));
        DevRefine r{};
        r.rows = d_rows;
        r.flags = x.d_flags.p;
        r.rids = x.d_rids.p;
        r.wrows = x.d_wrows.p;
        r.row_words = (uint32_t)nw;
        r.head = (uint32_t)rt | (uint32_t)pm << 16;
        r.tail = (uint32_t)st | (uint32_t)(uint16_t)(srel < 0 ? ACL_NO_RELATION : srel) << 16;
        r.fresh_sid = kFreshSubject;
        // a wildcard under an exclusion / intersection: every id of the type is a candidate (the complement of LookupSubjects' excluded row)
        ev_begin(c, 5);
        launch_refine_fill(c->stream, r, (uint32_t)wrows.size(), need, nobj, wid);
        ev_end(c);
        // the candidates' tile offsets: per-row totals for the slices
        const uint32_t ntiles = (uint32_t)((nw + kDiffTileWords - 1) / kDiffTileWords);
        const DevRowsDiff all{d_rows, d_rows, (uint32_t)nw, (uint32_t)nw, 0u, (uint32_t)W, nullptr};  // (old_nrows = 0: the old array is never read)
        uint64_t total = 0;
        rc = rows_diff_scan(c, all, x.d_counts, x.d_offs, 5, &total);
        if (rc) return rc;
        std::vector<uint64_t> offs((size_t)ntiles * W + 1);
        HIP_TRY(hipMemcpy(offs.data(), x.d_offs.p, offs.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
        const bool strict = !h->lenient_lookup;
        const uint64_t limit = std::max<uint32_t>(h->max_sub_batch, 1);
        size_t i0 = 0, f0 = 0;  // f0: the first of wrows at or behind row i0
        while (i0 < W) {
            // whole rows until the candidates (and stand-ins) reach max_sub_batch, at least one: subjects_batch's rule
            size_t i1 = i0, f1 = f0;
            uint64_t items = 0;
            for (; i1 < W && (i1 == i0 || items < limit); i1++) {
                items += offs[(i1 + 1) * ntiles] - offs[i1 * ntiles];
                if (f1 < wrows.size() && wrows[f1] == i1) items++, f1++;
            }
            const uint64_t nrec = offs[i1 * ntiles] - offs[i0 * ntiles];
            if (items > kWatchSetMaxChanges) return fail(ACL_ERR_RESOURCE_EXHAUSTED, "subject rows: more than 2^28 candidates in one row");
            if (items) {
                r.row0 = (uint32_t)i0;
                r.nrec = (uint32_t)nrec;
                r.wrow0 = (uint32_t)f0;
                r.nstand = (uint32_t)(f1 - f0);
                HIP_TRY(c->d_items.ensure(items));
                HIP_TRY(c->d_perm.ensure(items));
                HIP_TRY(c->d_errout.ensure(items));
                if (nrec) {
                    const DevRowsDiff d{d_rows, d_rows + i0 * nw, (uint32_t)nw, (uint32_t)nw, 0u, (uint32_t)(i1 - i0), nullptr};
                    if (i0) {  // (the first slice's offsets are the scan's own; a later slice's start from zero again)
                        ev_begin(c, 5);
                        launch_rows_diff_count(c->stream, d, x.d_counts.p, x.d_offs.p);
                        ev_end(c);
                    }
                    rc = rows_diff_emit(c, d, x.d_offs, x.d_recs, 5, nrec);
                    if (rc) return rc;
                }
                r.recs = x.d_recs.p;
                ev_begin(c, 5);
                launch_refine_items(c->stream, r, c->d_items.p);
                ev_end(c);
                rc = check_device(h, c, c->d_items.p, items, c->d_perm.p, c->d_errout.p);  // (ends with the stream synchronised)
                if (rc) return rc;
                HIP_TRY(c->h_out.ensure(64));
                HIP_TRY(hipMemsetAsync(x.d_status.p, 0xFF, sizeof(uint32_t), c->stream));
                ev_begin(c, 5);
                launch_refine_apply(c->stream, r, c->d_perm.p, c->d_errout.p, ACL_PERM_HAS_PERMISSION, x.d_status.p);
                ev_end(c);
                HIP_TRY(hipMemcpyAsync(c->h_out.p, x.d_status.p, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(hipStreamSynchronize(c->stream));
                ev_collect(c);
                const uint32_t first_err = *(const uint32_t *)c->h_out.p;
                if (first_err != 0xFFFFFFFFu && strict) {  // that one record: which subject on which resource, and how its Check failed
                    acl_item_t it;
                    int32_t code = 0;
                    HIP_TRY(hipMemcpy(&it, c->d_items.p + first_err, sizeof(it), hipMemcpyDeviceToHost));
                    HIP_TRY(hipMemcpy(&code, c->d_errout.p + first_err, sizeof(code), hipMemcpyDeviceToHost));
                    return subjects_error(code, it.resource_id, it.subject_id);
                }
            }
            i0 = i1;
            f0 = f1;
            rc = check_opts(c->opts);
            if (rc) return rc;
        }
    }
    if (!wrows.empty() && wid != 0xFFFFFFFFu) {
        ev_begin(c, 5);
        launch_refine_wild(c->stream, d_rows, (uint32_t)nw, x.d_flags.p, (uint32_t)W, wid);
        ev_end(c);
    }
    return ACL_OK;
}

static long row_of(const acl_watch_set *s, uint32_t watcher) {
    auto it = std::lower_bound(s->ids.begin(), s->ids.end(), watcher);
    return (it == s->ids.end() || *it != watcher) ? -1 : (long)(it - s->ids.begin());
}

static int set_poll(acl_engine *h, acl_watch_set *s, const CallOpts &opts, acl_watch_change_t **changes_out, size_t *n_out, uint64_t *revision_out) {
    std::lock_guard<std::mutex> lk(s->mu);
    s->polls++;
    int key_slot = -1;
    {
        std::shared_lock<RwLock> slk(h->state_mu);
        if (!h->store_only) {
            int rc = set_args_ok(h, s->rtype, s->perm, s->stype, s->srel);
            if (rc == ACL_OK) rc = not_sharded(h);  // (sharded since the set was opened: refused before the shard's snapshot is touched)
            if (rc) return rc;
            if (s->srel >= 0 && !s->subjects) key_slot = h->store.schema().slot(s->stype, s->srel);
        }
    }
    Eval ev;
    // (brings the snapshot up to date; a replica on the rows' device; the reverse rows for LookupResources' walk, the subject rows for LookupSubjects')
    int rc = ev.begin(h, !s->subjects, opts, key_slot, h->devs.size() > 1 ? s->device : -1, s->subjects);
    if (rc) return rc;
    rc = set_args_ok(h, s->rtype, s->perm, s->stype, s->srel);  // (the schema may have been reloaded in between)
    if (rc == ACL_OK) rc = not_sharded(h);
    if (rc) return rc;
    PassCtx *c = ev.c;
    const uint64_t epoch = h->snap_epoch;
    if (s->polled && !s->dirty && epoch == s->epoch) {  // nothing moved: no device work
        if (revision_out) *revision_out = s->revision;
        return ACL_OK;
    }
    const size_t W = s->ids.size();
    const uint32_t nobj = h->store.objects(s->row_type()).count();
    const size_t need = ((size_t)nobj + 31) / 32, nw = row_words_for(nobj);
    if ((W * nw + s->old_nrows * s->old_words) * sizeof(uint32_t) > kWatchSetBytes)
        return fail(ACL_ERR_RESOURCE_EXHAUSTED, "watch set: the row arrays would exceed 1 GiB of device memory (the type has grown): split the watchers over several sets");
    DevArray<uint32_t> &fresh = s->rows[s->cur ^ 1];
    size_t n = 0;
    acl_watch_change_t *recs = nullptr;
    if (W) {
        HIP_TRY(fresh.ensure(W * nw));
        rc = check_opts(opts);
        if (rc) return rc;
        s->walks++;
        const uint32_t target = (uint32_t)h->store.schema().slot(s->rtype, s->perm);
        if (s->subjects) {
            rc = subject_rows(h, c, s->rtype, s->perm, s->stype, s->srel, s->sids.data(), W, fresh.p, nw, s->subj);
            if (rc) return rc;
        } else if (h->snap.slot_nonmono.empty() || !h->snap.slot_nonmono[target]) {
            rc = lookup_batch(h, c, s->rtype, s->perm, s->stype, s->srel, s->sids.data(), W, nullptr, 0, nullptr, fresh.p, nw);
            if (rc) return rc;
        } else {
            // a permission with `&` / `-` / `.all()`: the walk's rows are candidates, confirmed by a forward Check on host rows (lookup_refine) -- the accepted
            // slow path: the refined rows go back up in one copy
            std::vector<uint32_t> host(W * nw);
            rc = lookup_batch(h, c, s->rtype, s->perm, s->stype, s->srel, s->sids.data(), W, host.data(), nw, nullptr);
            if (rc) return rc;
            HIP_TRY(hipMemcpy(fresh.p, host.data(), W * nw * sizeof(uint32_t), hipMemcpyHostToDevice));
        }
        rc = check_opts(opts);
        if (rc) return rc;
        HIP_TRY(s->d_ids.ensure(W));
        HIP_TRY(c->h_in.ensure(W * sizeof(uint32_t)));
        for (size_t i = 0; i < W; i++) ((uint32_t *)c->h_in.p)[i] = s->from_now[i] ? kDiffSkipRow : s->ids[i];
        HIP_TRY(hipMemcpyAsync(s->d_ids.p, c->h_in.p, W * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        const DevRowsDiff d{s->rows[s->cur].p, fresh.p, (uint32_t)s->old_words, (uint32_t)nw, (uint32_t)std::min(s->old_nrows, W), (uint32_t)W, s->d_ids.p};
        rc = rows_diff(c, d, s->d_counts, s->d_offs, s->d_recs, &recs, &n);
        if (rc) return rc;
        if (s->subjects) {  // the record of the wildcard object's bit says so
            const uint32_t wid = h->store.wildcard_id(s->stype);
            for (size_t k = 0; k < n; k++)
                if (recs[k].resource_id == wid) recs[k].reserved = ACL_WATCH_CHANGE_WILDCARD;
        }
        s->cur ^= 1;  // the fresh rows are the baseline from here on
    }
    s->old_words = nw;
    s->old_need = need;
    s->old_nrows = W;
    std::fill(s->from_now.begin(), s->from_now.end(), (uint8_t)0);
    s->polled = true;
    s->dirty = false;
    s->epoch = epoch;
    s->revision = h->snap.revision;
    s->changes += n;
    *changes_out = recs;
    *n_out = n;
    if (revision_out) *revision_out = s->revision;
    return ACL_OK;
}

void watch_sets_release(acl_engine_t *h) {
    std::vector<acl_watch_set *> sets;
    {
        std::lock_guard<std::mutex> lk(h->watch_sets_mu);
        sets.swap(h->watch_sets);
    }
    for (acl_watch_set *s : sets) delete s;
}

static int known_set(acl_engine *h, acl_watch_set *s) {
    if (!h || !s) return fail(ACL_ERR_INVALID_ARGUMENT, "watch set: NULL handle");
    std::lock_guard<std::mutex> lk(h->watch_sets_mu);
    if (std::find(h->watch_sets.begin(), h->watch_sets.end(), s) == h->watch_sets.end()) return fail(ACL_ERR_INVALID_ARGUMENT, "watch set: not an open set of this engine");
    return ACL_OK;
}

}  // namespace aclint

extern "C" {

static int set_open(acl_engine_t *h, int rtype, int permission, int stype, int srel, bool subjects, acl_watch_set_t **out) {
    if (!h || !out) return fail(ACL_ERR_INVALID_ARGUMENT, subjects ? "acl_watch_set_open_subjects: NULL argument" : "acl_watch_set_open: NULL argument");
    *out = nullptr;
    {
        std::shared_lock<RwLock> slk(h->state_mu);
        int rc = set_args_ok(h, rtype, permission, stype, srel);
        if (rc) return rc;
        if (subjects) rc = not_sharded(h);  // (one shard of a graph is refused as such, with or without a device)
        if (rc) return rc;
        if (h->store_only) return fail(ACL_ERR_UNAVAILABLE, "engine was opened store-only (no GPU): watch sets are unavailable");
        rc = not_sharded(h);
        if (rc) return rc;
    }
    auto s = std::make_unique<acl_watch_set>();
    s->rtype = rtype;
    s->perm = permission;
    s->stype = stype;
    s->srel = srel;
    s->subjects = subjects;
    {
        std::lock_guard<std::mutex> lk(h->pool_mu);  // (next_dev: where evaluations are spread from, too)
        s->device = h->devs[h->devs.size() > 1 ? h->next_dev++ % h->devs.size() : 0]->device;
    }
    std::lock_guard<std::mutex> lk(h->watch_sets_mu);
    h->watch_sets.push_back(s.get());
    *out = s.release();
    return ACL_OK;
}

int acl_watch_set_open(acl_engine_t *h, int rtype, int permission, int stype, int srel, acl_watch_set_t **out) {
    return set_open(h, rtype, permission, stype, srel, false, out);
}

int acl_watch_set_open_subjects(acl_engine_t *h, int rtype, int permission, int stype, int srel, acl_watch_set_t **out) {
    return set_open(h, rtype, permission, stype, srel, true, out);
}

int acl_watch_set_add(acl_engine_t *h, acl_watch_set_t *s, const char *subject_id, uint32_t flags, uint32_t *watcher_out) {
    int rc = known_set(h, s);
    if (rc) return rc;
    if (empty(subject_id) || !watcher_out || (flags & ~ACL_WATCHER_FROM_NOW)) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_watch_set_add: bad argument");
    if (!valid_object_id(subject_id)) return fail(ACL_ERR_INVALID_ARGUMENT, std::string("acl_watch_set_add: `") + subject_id + "` does not match the API's object id pattern");
    std::lock_guard<std::mutex> lk(s->mu);
    std::shared_lock<RwLock> slk(h->state_mu);
    std::unique_lock<std::shared_mutex> nlk(h->names_mu);
    rc = set_args_ok(h, s->rtype, s->perm, s->stype, s->srel);
    if (rc) return rc;
    if (s->next_id == kDiffSkipRow) return fail(ACL_ERR_RESOURCE_EXHAUSTED, "acl_watch_set_add: watcher ids exhausted");
    const size_t nw = row_words_for(h->store.objects(s->row_type()).count());
    if ((s->ids.size() + 1) * nw * 2 * sizeof(uint32_t) > kWatchSetBytes)
        return fail(ACL_ERR_RESOURCE_EXHAUSTED, "acl_watch_set_add: the set's two row arrays would exceed 1 GiB of device memory: open another set");
    // pinned, as acl_intern: somebody who watches before the first grant has no relationship, and the watch lives for hours -- the id must not be recycled under it
    // (a subject-direction set watches a resource: the same holds for its id)
    const uint32_t sid = h->store.intern_object(s->watched_type(), subject_id, true);
    s->ids.push_back(s->next_id);
    s->sids.push_back(sid);
    s->from_now.push_back((flags & ACL_WATCHER_FROM_NOW) ? 1 : 0);
    s->dirty = true;
    *watcher_out = s->next_id++;
    return ACL_OK;
}

int acl_watch_set_remove(acl_engine_t *h, acl_watch_set_t *s, uint32_t watcher) {
    int rc = known_set(h, s);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(s->mu);
    const long r = row_of(s, watcher);
    if (r < 0) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_watch_set_remove: unknown watcher");
    if ((size_t)r < s->old_nrows) {  // close the gap in the baseline: the rows behind it move up by one, through the scratch array (the regions overlap)
        const size_t tail = (s->old_nrows - 1 - (size_t)r) * s->old_words;
        if (tail) {
            HIP_TRY(hipSetDevice(s->device));
            DevArray<uint32_t> &old = s->rows[s->cur], &tmp = s->rows[s->cur ^ 1];
            HIP_TRY(tmp.ensure(tail));
            HIP_TRY(hipMemcpy(tmp.p, old.p + ((size_t)r + 1) * s->old_words, tail * sizeof(uint32_t), hipMemcpyDeviceToDevice));
            HIP_TRY(hipMemcpy(old.p + (size_t)r * s->old_words, tmp.p, tail * sizeof(uint32_t), hipMemcpyDeviceToDevice));
        }
        s->old_nrows--;
    }
    s->ids.erase(s->ids.begin() + r);
    s->sids.erase(s->sids.begin() + r);
    s->from_now.erase(s->from_now.begin() + r);
    return ACL_OK;
}

int acl_watch_set_poll(acl_engine_t *h, acl_watch_set_t *s, const acl_call_opts_t *o, acl_watch_change_t **changes_out, size_t *n_out, uint64_t *revision_out) {
    int rc = known_set(h, s);
    if (rc) return rc;
    if (!changes_out || !n_out) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_watch_set_poll: NULL output");
    *changes_out = nullptr;
    *n_out = 0;
    const CallOpts opts = call_opts(o);
    return set_poll(h, s, opts, changes_out, n_out, revision_out);
}

int acl_watch_set_row(acl_engine_t *h, acl_watch_set_t *s, uint32_t watcher, uint32_t *bitmap_out, size_t words) {
    int rc = known_set(h, s);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(s->mu);
    const long r = row_of(s, watcher);
    if (r < 0) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_watch_set_row: unknown watcher");
    const bool have = (size_t)r < s->old_nrows;  // (else: added since the last poll -- the empty row)
    if ((words && !bitmap_out) || (have && words < s->old_need))
        return fail(ACL_ERR_INVALID_ARGUMENT, "acl_watch_set_row: bitmap too small (" + std::to_string(s->old_need) + " words needed)");
    const size_t cw = have ? std::min(words, s->old_words) : 0;
    if (cw) {
        HIP_TRY(hipSetDevice(s->device));
        HIP_TRY(hipMemcpy(bitmap_out, s->rows[s->cur].p + (size_t)r * s->old_words, cw * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    std::fill(bitmap_out + cw, bitmap_out + words, 0u);
    return ACL_OK;
}

int acl_watch_set_stats(acl_engine_t *h, acl_watch_set_t *s, uint64_t *polls, uint64_t *walks, uint64_t *changes) {
    int rc = known_set(h, s);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(s->mu);
    if (polls) *polls = s->polls;
    if (walks) *walks = s->walks;
    if (changes) *changes = s->changes;
    return ACL_OK;
}

int acl_watch_set_close(acl_engine_t *h, acl_watch_set_t *s) {
    if (!h || !s) return fail(ACL_ERR_INVALID_ARGUMENT, "watch set: NULL handle");
    {
        std::lock_guard<std::mutex> lk(h->watch_sets_mu);
        auto it = std::find(h->watch_sets.begin(), h->watch_sets.end(), s);
        if (it == h->watch_sets.end()) return fail(ACL_ERR_INVALID_ARGUMENT, "watch set: not an open set of this engine");
        h->watch_sets.erase(it);
    }
    { std::lock_guard<std::mutex> lk(s->mu); }  // (a poll in flight finishes first; no call on a set may be started after its close)
    delete s;
    return ACL_OK;
}

int acl_selfcheck_rows_diff(acl_engine_t *h, const uint32_t *old_rows, size_t old_words, const uint32_t *new_rows, size_t new_words, size_t n_rows,
                            acl_watch_change_t **changes_out, size_t *n_out) {
    if (!h || !changes_out || !n_out || (n_rows && ((old_words && !old_rows) || (new_words && !new_rows))) || old_words > (1u << 27) || new_words > (1u << 27) ||
        n_rows > 0x7FFFFFFFull)
        return fail(ACL_ERR_INVALID_ARGUMENT, "acl_selfcheck_rows_diff: bad argument");
    *changes_out = nullptr;
    *n_out = 0;
    Eval ev;
    int rc = ev.begin(h, false);
    if (rc) return rc;
    DevArray<uint32_t> d_old, d_new, d_counts;
    DevArray<uint64_t> d_offs;
    DevArray<uint4> d_recs;
    HIP_TRY(d_old.ensure(n_rows * old_words));
    HIP_TRY(d_new.ensure(n_rows * new_words));
    if (n_rows * old_words) HIP_TRY(hipMemcpy(d_old.p, old_rows, n_rows * old_words * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (n_rows * new_words) HIP_TRY(hipMemcpy(d_new.p, new_rows, n_rows * new_words * sizeof(uint32_t), hipMemcpyHostToDevice));
    const DevRowsDiff d{d_old.p, d_new.p, (uint32_t)old_words, (uint32_t)new_words, (uint32_t)n_rows, (uint32_t)n_rows, nullptr};
    return rows_diff(ev.c, d, d_counts, d_offs, d_recs, changes_out, n_out);
}

int acl_selfcheck_subject_rows(acl_engine_t *h, int rtype, int permission, int stype, int srel, const uint32_t *resource_ids, size_t n, uint32_t *bitmaps_out,
                               size_t words) {
    if (!h || (n && (!resource_ids || !bitmaps_out))) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_selfcheck_subject_rows: NULL argument");
    {
        std::shared_lock<RwLock> slk(h->state_mu);
        int rc = set_args_ok(h, rtype, permission, stype, srel);
        if (rc) return rc;
        if (h->store_only) return fail(ACL_ERR_UNAVAILABLE, "engine was opened store-only (no GPU): watch sets are unavailable");
        rc = not_sharded(h);
        if (rc) return rc;
    }
    Eval ev;
    int rc = ev.begin(h, false, CallOpts(), -1, -1, true);
    if (rc) return rc;
    rc = set_args_ok(h, rtype, permission, stype, srel);
    if (rc == ACL_OK) rc = not_sharded(h);
    if (rc) return rc;
    const uint32_t nobj = h->store.objects(stype).count();
    const size_t need = ((size_t)nobj + 31) / 32, nw = row_words_for(nobj);
    if (words < need) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_selfcheck_subject_rows: bitmap too small (" + std::to_string(need) + " words needed)");
    if (n * nw * sizeof(uint32_t) > kWatchSetBytes / 2) return fail(ACL_ERR_RESOURCE_EXHAUSTED, "acl_selfcheck_subject_rows: more than 512 MiB of rows");
    if (!n) return ACL_OK;
    SubjScratch x;
    DevArray<uint32_t> d_rows;
    HIP_TRY(d_rows.ensure(n * nw));
    rc = subject_rows(h, ev.c, rtype, permission, stype, srel, resource_ids, n, d_rows.p, nw, x);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(ev.c->stream));
    ev_collect(ev.c);
    const size_t cw = std::min(words, nw);
    HIP_TRY(hipMemcpy2D(bitmaps_out, words * sizeof(uint32_t), d_rows.p, nw * sizeof(uint32_t), cw * sizeof(uint32_t), n, hipMemcpyDeviceToHost));
    if (words > cw)
        for (size_t i = 0; i < n; i++) std::fill(bitmaps_out + i * words + cw, bitmaps_out + (i + 1) * words, 0u);
    return ACL_OK;
}

}  // extern "C"

// engine_subjects.cpp -- LookupSubjects (include/aclgpu.h acl_lookup_subjects*): who holds a permission on one resource.
//
// The device walks the forward programs from the resource (kernels.hip k_subj_local) over the subject rows (plan_subjects.cpp), one block per resource.
// What it returns per resource is exact for a monotone permission: a Check finds a subject iff some path of the programs reaches a row that names it
// within the dispatch-depth limit, and that is what the walk marks.  A permission whose value can depend on `-`, `&` or `.all()` (Snapshot::slot_nonmono)
// is walked by its positive relaxation: the row holds CANDIDATES, confirmed by one batched forward Check -- the way LookupResources confirms its own
// (engine_lookup.cpp lookup_refine) -- and a candidate whose Check errs fails the call with ACL_ERR_DEPTH (ACL_FLAG_LENIENT_LOOKUP: it is left out).
// `T:*` rows reached by the walk raise the answer's wildcard flag: "every subject of T, except the excluded row".
#include "engine_internal.hpp"
#include "validate.hpp"

namespace aclint {

namespace {

constexpr uint32_t kSubjCapFirst = 1u << 14;     // log entries per block of the first attempt (128 KiB)
constexpr uint32_t kSubjCapMax = 1u << 24;       // ... and at most (128 MiB): beyond, ACL_ERR_RESOURCE_EXHAUSTED

}  // namespace

int subjects_error(int32_t code, uint32_t rid, uint32_t sid) {
    const std::string who = sid == kFreshSubject ? std::string("the wildcard (a subject no relationship names)") : "subject id " + std::to_string(sid);
    return fail(code, std::string(code == ACL_ERR_DEPTH ? "LookupSubjects: max depth exceeded" : "LookupSubjects: a subject's check failed") + " while checking " + who +
                          " on resource id " + std::to_string(rid) + " (the permission holds an intersection / exclusion: reached subjects are confirmed by a forward Check)");
}

namespace {

// one launch per group of resources: rows of `row_words` words into bitmaps (stride `words`), wildcard reached into wild[].  With `dev` (subject-direction
// watch sets) the rows stay on the device instead: a chunk whose status is good is copied from d_subj_rows to dev->rows + (b + i) * dev->stride, the words
// behind row_words zeroed, and its flag words to dev->flags + b -- a chunk that is walked again with a larger log has written nothing there yet
int subjects_walk(acl_engine *h, PassCtx *c, uint32_t target, uint32_t key, const uint32_t *rids, size_t n, uint32_t *bitmaps, size_t words, size_t row_words,
                  uint8_t *wild, const SubjDevDst *dev = nullptr) {
    const DevSubjects g = dev_subjects(h, c);
    const BlockWalk w{"LookupSubjects", "resource", 2 /* (8-byte log entries) */, row_words, kSubjCapFirst, kSubjCapMax};
    uint32_t *h_rows = nullptr, *h_flags = nullptr;
    return block_walk_chunks(
        h, c, w, n,
        [&](size_t b, size_t m) {
            HIP_TRY(c->d_sids.ensure(m));
            HIP_TRY(c->d_subj_rows.ensure(std::max<size_t>(m * row_words, 1)));
            HIP_TRY(c->d_subj_flags.ensure(m));
            HIP_TRY(c->h_in.ensure(m * sizeof(uint32_t)));
            HIP_TRY(c->h_out.ensure(std::max<size_t>(dev ? 0 : m * row_words, 1) * 4 + m * 4));
            std::memcpy(c->h_in.p, rids + b, m * sizeof(uint32_t));
            HIP_TRY(hipMemcpyAsync(c->d_sids.p, c->h_in.p, m * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
            if (row_words) HIP_TRY(hipMemsetAsync(c->d_subj_rows.p, 0, m * row_words * 4, c->stream));
            return (int)ACL_OK;
        },
        [&](size_t m, uint32_t cap) {
            ev_begin(c, 4);
            launch_subj_local(c->stream, g, c->d_sids.p, (uint32_t)m, target, key, c->d_fbuf[0].p, cap, c->d_subj_visited.p, c->d_subj_rows.p, (uint32_t)row_words,
                              c->d_subj_flags.p, c->d_status.p);
            ev_end(c);
            HIP_TRY(hipGetLastError());
            h_rows = (uint32_t *)c->h_out.p;
            h_flags = h_rows + (dev ? 0 : m * row_words);
            if (row_words && !dev) HIP_TRY(hipMemcpyAsync(h_rows, c->d_subj_rows.p, m * row_words * 4, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipMemcpyAsync(h_flags, c->d_subj_flags.p, m * 4, hipMemcpyDeviceToHost, c->stream));
            return (int)ACL_OK;
        },
        [&](size_t b, size_t m) {
            if (dev) {
                // (one strided copy kernel: a 2-D runtime copy of narrow rows costs a launch per row)
                ev_begin(c, 4);
                launch_subj_rows_store(c->stream, c->d_subj_rows.p, (uint32_t)row_words, c->d_subj_flags.p, (uint32_t)m, dev->rows + b * dev->stride, (uint32_t)dev->stride,
                                       dev->flags + b);
                ev_end(c);
                HIP_TRY(hipGetLastError());
                for (size_t i = 0; i < m; i++) wild[b + i] = h_flags[i] ? 1 : 0;
                return (int)ACL_OK;
            }
            for (size_t i = 0; i < m; i++) {
                uint32_t *dst = bitmaps + (b + i) * words;
                if (row_words) std::memcpy(dst, h_rows + i * row_words, row_words * 4);
                std::fill(dst + row_words, dst + words, 0u);
                wild[b + i] = h_flags[i] ? 1 : 0;
            }
            return (int)ACL_OK;
        });
}

// forward Checks of (rt, pm) @ (st, srel) over `items`' subjects, in chunks: answers / errors by index
int check_items(acl_engine *h, PassCtx *c, std::vector<acl_item_t> &items, std::vector<uint8_t> *perm, std::vector<int32_t> *err) {
    perm->assign(items.size(), 0);
    err->assign(items.size(), 0);
    return check_ids_chunked(h, c, items.data(), items.size(), perm->data(), err->data());
}

}  // namespace

// caller holds an Eval (snapshot + subject rows current) and validated the arguments
int subjects_batch(acl_engine *h, PassCtx *c, int rt, int pm, int st, int srel, const uint32_t *rids, size_t n, uint32_t *bitmaps, size_t words, uint64_t *counts,
                   uint8_t *flags, uint32_t *excluded) {
    int rc = not_sharded(h);
    if (rc) return rc;
    const Schema &sc = h->store.schema();
    const uint32_t target = (uint32_t)sc.slot(rt, pm);
    const uint32_t key = sc.subject_key(st, srel < 0 ? kNoRelation : srel);
    const uint32_t nobj = h->store.objects(st).count();
    const size_t need = ((size_t)nobj + 31) / 32;
    if (words < need)
        return fail_detail(ACL_ERR_INVALID_ARGUMENT, kDetailBitmapTooSmall, "lookup_subjects: bitmap too small (" + std::to_string(need) + " words needed)");
    const uint32_t nres = h->store.objects(rt).count();
    for (size_t i = 0; i < n; i++)
        if (rids[i] >= nres) return fail(ACL_ERR_INVALID_ARGUMENT, "lookup_subjects: resource id " + std::to_string(rids[i]) + " beyond the type's objects");
    std::vector<uint8_t> wild(n, 0);
    rc = subjects_walk(h, c, target, key, rids, n, bitmaps, words, need, wild.data());
    if (rc) return rc;
    c->stats.lookup_requests += n;
    const bool nonmono = h->snap.slot_nonmono.size() > target && h->snap.slot_nonmono[target];
    const bool strict = !h->lenient_lookup;
    const uint16_t sr = (uint16_t)(srel < 0 ? ACL_NO_RELATION : srel);
    std::vector<acl_item_t> items;
    std::vector<uint8_t> perm;
    std::vector<int32_t> err;
    if (nonmono) {
        // candidates + the wildcard's stand-in (a subject nobody names), one batched forward Check per bounded slice of lookups
        const size_t limit = std::max<size_t>(h->max_sub_batch, 1);
        size_t i0 = 0;
        while (i0 < n) {
            items.clear();
            size_t i1 = i0;
            for (; i1 < n && (i1 == i0 || items.size() < limit); i1++) {
                const uint32_t *row = bitmaps + i1 * words;
                for (size_t w = 0; w < need; w++)
                    for (uint32_t mm = row[w]; mm; mm &= mm - 1)
                        items.push_back(acl_item_t{(uint16_t)rt, (uint16_t)pm, rids[i1], (uint16_t)st, sr, (uint32_t)(w * 32 + (size_t)__builtin_ctz(mm))});
                if (wild[i1]) items.push_back(acl_item_t{(uint16_t)rt, (uint16_t)pm, rids[i1], (uint16_t)st, sr, kFreshSubject});
            }
            rc = check_items(h, c, items, &perm, &err);
            if (rc) return rc;
            size_t k = 0;
            for (size_t i = i0; i < i1; i++) {
                uint32_t *row = bitmaps + i * words;
                for (size_t w = 0; w < need; w++)
                    for (uint32_t mm = row[w]; mm; mm &= mm - 1, k++) {
                        if (err[k] && strict) return subjects_error(err[k], rids[i], items[k].subject_id);
                        if (err[k] || perm[k] != ACL_PERM_HAS_PERMISSION) row[w] &= ~(mm & (0u - mm));
                    }
                if (wild[i]) {
                    if (err[k] && strict) return subjects_error(err[k], rids[i], kFreshSubject);
                    wild[i] = !err[k] && perm[k] == ACL_PERM_HAS_PERMISSION;
                    k++;
                }
            }
            i0 = i1;
            rc = check_opts(c->opts);
            if (rc) return rc;
        }
    }
    if (excluded) {
        for (size_t i = 0; i < n; i++) {
            uint32_t *ex = excluded + i * words;
            std::fill(ex, ex + words, 0u);
            if (!wild[i] || !nonmono) continue;  // (a monotone permission that a wildcard grants excludes nobody)
            // every subject of the type: who does NOT hold it (a subject whose Check errs does not hold it either; strict: the call fails).
            // The wildcard's own id (the name "*") is not a subject.
            const uint32_t wid = h->store.wildcard_id(st);
            const size_t chunk = std::min<size_t>(std::max<size_t>(h->max_sub_batch, 1), 262144);
            for (size_t s0 = 0; s0 < nobj; s0 += chunk) {
                const size_t m = std::min<size_t>(chunk, nobj - s0);
                items.resize(m);
                for (size_t j = 0; j < m; j++) items[j] = acl_item_t{(uint16_t)rt, (uint16_t)pm, rids[i], (uint16_t)st, sr, (uint32_t)(s0 + j)};
                rc = check_items(h, c, items, &perm, &err);
                if (rc) return rc;
                for (size_t j = 0; j < m; j++) {
                    if (s0 + j == wid) continue;
                    if (err[j] && strict) return subjects_error(err[j], rids[i], (uint32_t)(s0 + j));
                    if (err[j] || perm[j] != ACL_PERM_HAS_PERMISSION) ex[(s0 + j) >> 5] |= 1u << ((s0 + j) & 31u);
                }
                rc = check_opts(c->opts);
                if (rc) return rc;
            }
        }
    }
    for (size_t i = 0; i < n; i++) {
        if (counts) counts[i] = popcount_words(bitmaps + i * words, need);
        if (flags) flags[i] = wild[i] ? (uint8_t)ACL_SUBJECTS_WILDCARD : (uint8_t)0;
    }
    return ACL_OK;
}

namespace {

int subjects_args_ok(acl_engine *h, int rt, int pm, int st, int srel) {
    const Schema &sc = h->store.schema();
    if (rt < 0 || rt >= (int)sc.defs.size() || st < 0 || st >= (int)sc.defs.size() || pm < 0 || pm >= (int)sc.defs[rt].members.size() ||
        srel >= (int)sc.defs[st].members.size())
        return fail(ACL_ERR_FAILED_PRECONDITION, "lookup_subjects: unknown type, permission or subject relation");
    return ACL_OK;
}

int subjects_batch_call(acl_engine_t *h, int rt, int pm, int st, int srel, const uint32_t *rids, size_t n, uint32_t *bitmaps, size_t words, uint64_t *counts,
                        uint8_t *flags, uint32_t *excluded, const CallOpts &opts) {
    if (n && (!rids || !bitmaps)) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_lookup_subjects_batch: NULL buffer");
    {
        std::shared_lock<RwLock> slk(h->state_mu);
        if (!h->store_only) {
            if (!h->store.has_schema()) return fail(ACL_ERR_FAILED_PRECONDITION, "no schema loaded");
            int rc = subjects_args_ok(h, rt, pm, st, srel);
            if (rc) return rc;
            rc = not_sharded(h);
            if (rc) return rc;
        }
    }
    Eval ev;
    int rc = ev.begin(h, false, opts, -1, -1, true);
    if (rc) return rc;
    rc = subjects_args_ok(h, rt, pm, st, srel);  // (the schema may have been reloaded in between)
    if (rc) return rc;
    return subjects_batch(h, ev.c, rt, pm, st, srel, rids, n, bitmaps, words, counts, flags, excluded);
}

}  // namespace

int subjects_walk_device(acl_engine *h, PassCtx *c, int rt, int pm, int st, int srel, const uint32_t *rids, size_t n, const SubjDevDst &dst, uint8_t *wild) {
    int rc = not_sharded(h);
    if (rc) return rc;
    const Schema &sc = h->store.schema();
    const uint32_t nres = h->store.objects(rt).count();
    for (size_t i = 0; i < n; i++)
        if (rids[i] >= nres) return fail(ACL_ERR_INVALID_ARGUMENT, "lookup_subjects: resource id " + std::to_string(rids[i]) + " beyond the type's objects");
    const size_t need = ((size_t)h->store.objects(st).count() + 31) / 32;
    if (dst.stride < need) return fail(ACL_ERR_INTERNAL, "subject rows: the destination's rows are narrower than the type's ids");
    rc = subjects_walk(h, c, (uint32_t)sc.slot(rt, pm), sc.subject_key(st, srel < 0 ? kNoRelation : srel), rids, n, nullptr, 0, need, wild, &dst);
    if (rc) return rc;
    c->stats.lookup_requests += n;
    return ACL_OK;
}

bool subjects_current(acl_engine *h) {
    const SubjectRows &s = h->subj;
    if (s.epoch != h->snap_epoch) return false;
    for (const auto &d : h->devs)
        if (d->subj_epoch != s.epoch) return false;
    const Schema &sc = h->store.schema();
    if (s.slot_vbase.size() != (size_t)sc.nslots) return false;
    // (ids interned since the build have no relationships in this snapshot, but a state of theirs -- a lookup's own resource -- must fit the visited bits)
    for (int slot = 0; slot < sc.nslots; slot++)
        if (s.slot_vbase[slot] != kSubjNoBits && h->store.objects(sc.slot_owner[slot].first).count() > s.slot_vn[slot]) return false;
    return true;
}

int ensure_subjects(acl_engine *h) {
    if (subjects_current(h)) return ACL_OK;
    for (auto &dp : h->devs) dp->subj_epoch = ~0ull;
    build_subjects(h->store, h->store.now(), h->snap, &h->subj);
    h->subj.epoch = h->snap_epoch;
    for (auto &dp : h->devs) {
        DevState &d = *dp;
        hipStream_t s = d.up_stream;
        HIP_TRY(hipSetDevice(d.device));
        HIP_TRY(d.d_smeta.upload(h->subj.smeta, s));
        HIP_TRY(d.d_sids.upload(h->subj.sids, s));
        HIP_TRY(d.d_sops.upload(h->subj.sops, s));
        HIP_TRY(d.d_svbase.upload(h->subj.slot_vbase, s));
        HIP_TRY(d.d_svn.upload(h->subj.slot_vn, s));
    }
    for (auto &dp : h->devs) {
        HIP_TRY(hipSetDevice(dp->device));
        HIP_TRY(hipStreamSynchronize(dp->up_stream));
        dp->subj_epoch = h->subj.epoch;
    }
    std::lock_guard<std::mutex> lk(h->stats_mu);
    h->stats.snapshot_bytes += h->subj.bytes();
    return ACL_OK;
}

}  // namespace aclint

int acl_lookup_subjects_batch(acl_engine_t *h, int rtype, int perm, int stype, int srel, const uint32_t *resource_ids, size_t n, uint32_t *bitmaps, size_t words,
                              uint64_t *counts, uint8_t *flags, uint32_t *excluded, const acl_call_opts_t *opts) {
    return subjects_batch_call(h, rtype, perm, stype, srel, resource_ids, n, bitmaps, words, counts, flags, excluded, call_opts(opts));
}

int acl_lookup_subjects(acl_engine_t *h, const char *rtype, const char *rid, const char *perm, const char *stype, const char *srel, const acl_call_opts_t *o,
                        uint32_t **bitmap_out, size_t *words_out, uint64_t *count_out, int *wildcard_out, uint32_t **excluded_out) {
    if (!bitmap_out || !words_out) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_lookup_subjects: NULL output");
    *bitmap_out = nullptr;
    *words_out = 0;
    if (excluded_out) *excluded_out = nullptr;
    if (count_out) *count_out = 0;
    if (wildcard_out) *wildcard_out = 0;
    if (empty(rtype) || empty(rid) || empty(perm) || empty(stype)) return fail(ACL_ERR_INVALID_ARGUMENT, "invalid LookupSubjectsRequest: empty field");
    const CallOpts opts = call_opts(o);
    int rt = -1, pm = -1, st = -1, sr = -1;
    bool known = false;
    uint32_t res = 0;
    {
        std::shared_lock<RwLock> slk(h->state_mu);
        std::shared_lock<std::shared_mutex> nlk(h->names_mu);
        if (!h->store.has_schema()) return fail(ACL_ERR_FAILED_PRECONDITION, "no schema loaded");
        const Schema &sc = h->store.schema();
        rt = sc.type_of(rtype);
        st = sc.type_of(stype);
        const bool srel_given = !empty(srel) && std::strcmp(srel, "...") != 0;
        // API validation first (validate.hpp), as for LookupResources; `*` is not a resource id
        if ((rt < 0 && !valid_type_name(rtype)) || (st < 0 && !valid_type_name(stype)) || ((rt < 0 || sc.defs[rt].find(perm) < 0) && !valid_relation_name(perm)) ||
            (srel_given && (st < 0 || sc.defs[st].find(srel) < 0) && !valid_relation_name(srel)) || !valid_object_id(rid))
            return fail(ACL_ERR_INVALID_ARGUMENT, "invalid LookupSubjectsRequest: a field does not match the API's pattern");
        if (rt < 0) return fail(ACL_ERR_FAILED_PRECONDITION, std::string("object definition `") + rtype + "` not found");
        pm = sc.defs[rt].find(perm);
        if (pm < 0) return fail(ACL_ERR_FAILED_PRECONDITION, std::string("relation/permission `") + perm + "` not found under definition `" + rtype + "`");
        if (st < 0) return fail(ACL_ERR_FAILED_PRECONDITION, std::string("object definition `") + stype + "` not found");
        if (srel_given) {
            sr = sc.defs[st].find(srel);
            if (sr < 0) return fail(ACL_ERR_FAILED_PRECONDITION, std::string("relation `") + srel + "` not found under definition `" + stype + "`");
        }
        if (h->store_only) return fail(ACL_ERR_UNAVAILABLE, "engine was opened store-only (no GPU): LookupSubjects is unavailable");
        int rc = not_sharded(h);
        if (rc) return rc;
        known = h->store.objects(rt).find(rid, &res);
        if (known) h->store.touch(rt, res);
    }
    const bool want_ex = excluded_out != nullptr;
    return owned_bitmap_retry("lookup_subjects: the object table kept growing faster than the result bitmap", [&]() -> int {
        const size_t words = owned_bitmap_words(h, st);
        uint32_t *bm = (uint32_t *)std::calloc(std::max<size_t>(words, 1), sizeof(uint32_t));
        uint32_t *ex = want_ex ? (uint32_t *)std::calloc(std::max<size_t>(words, 1), sizeof(uint32_t)) : nullptr;
        if (!bm || (want_ex && !ex)) {
            std::free(bm);
            std::free(ex);
            return fail(ACL_ERR_RESOURCE_EXHAUSTED, "out of host memory for the result bitmap");
        }
        uint64_t count = 0;
        uint8_t flag = 0;
        // (an unknown resource has no relationships: the empty answer, without a walk)
        const int rc = known ? subjects_batch_call(h, rt, pm, st, sr, &res, 1, bm, words, &count, &flag, ex, opts) : ACL_OK;
        if (rc == ACL_OK) {
            *bitmap_out = bm;
            *words_out = words;
            if (count_out) *count_out = count;
            if (wildcard_out) *wildcard_out = (flag & ACL_SUBJECTS_WILDCARD) ? 1 : 0;
            if (want_ex) {
                if (flag & ACL_SUBJECTS_WILDCARD) *excluded_out = ex;
                else std::free(ex);
            }
            return ACL_OK;
        }
        std::free(bm);
        std::free(ex);
        return rc;
    });
}

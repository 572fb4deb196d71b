// engine_lookup_multi.cpp -- LookupResources against MANY (type, permission) targets: one reverse walk per subject hands back every target's row
// (kernels.hip k_rev_multi).  The per-target loop over lookup_batch (engine_lookup.cpp) is the fallback and the definition of the answer.
#include "engine_internal.hpp"
#include "validate.hpp"

namespace aclint {

namespace {

struct MultiTargets {
    std::vector<RevMultiTarget> dev;  // what the kernel reads: {slot, out_off, copy_words, out_words}
    std::vector<size_t> off;          // first word of target j's row inside a subject's stride
    size_t stride = 0, copy_total = 0;
    RevUseful useful, is_target;
    bool any_nonmono = false;
};

// The one launch over m subjects already in `sids` (host).  Rows and counts in the caller's layout.  kTakeLevelLoop: a block gave up, or the group does not fit.
int multi_pass_local(acl_engine *h, PassCtx *c, const DevReverse &r, uint32_t key, const MultiTargets &mt, const uint32_t *sids, size_t m, uint32_t *bitmaps, uint64_t *counts) {
    const size_t T = mt.dev.size();
    if (mt.stride > 0xFFFFFFFFull || T > 0xFFFFFFFFull) return kTakeLevelLoop;
    const bool direct = mt.stride && h->is_pinned(bitmaps, m * mt.stride * sizeof(uint32_t));
    RevPass p;  // (rows in the staging: m x stride words)
    int rc = rev_pass_begin(h, c, m, m * T, direct ? 0 : m * std::max<size_t>(mt.stride, 1) * 4, true, &p);
    if (rc) return rc;
    // pinned input: [sids m x 4, padded to 16] [targets T x 16]
    const size_t tg_off = (m * sizeof(uint32_t) + 15) / 16 * 16;
    HIP_TRY(c->h_in.ensure(tg_off + T * sizeof(RevMultiTarget)));
    std::memcpy(c->h_in.p, sids, m * sizeof(uint32_t));
    std::memcpy((char *)c->h_in.p + tg_off, mt.dev.data(), T * sizeof(RevMultiTarget));
    void *d_rows = p.d_rows;
    if (direct) HIP_TRY(hipHostGetDevicePointer(&d_rows, bitmaps, 0));
    ev_begin(c, 6);
    launch_rev_multi(c->stream, r, (const uint32_t *)c->h_in.dp, (uint32_t)m, key, (const RevMultiTarget *)((const char *)c->h_in.dp + tg_off), (uint32_t)T, c->d_fbuf[0].p,
                     p.cap, (uint32_t *)d_rows, (uint32_t)mt.stride, p.d_counts, p.d_status, mt.useful, mt.is_target, p.spin ? c->d_done.p : nullptr, p.d_done_flag, p.done_val);
    ev_end(c);
    rc = rev_pass_end(c, p, counts);
    if (rc) return rc;
    if (!direct && mt.stride) std::memcpy(bitmaps, p.h_rows, m * mt.stride * 4);
    c->stats.rev_multi_passes++;
    c->stats.lookup_requests += m * T;
    return ACL_OK;
}

int multi_args_ok(acl_engine *h, const acl_target_t *targets, size_t T, int stype, int srel, const size_t *row_words) {
    const Schema &sc = h->store.schema();
    if (stype < 0 || stype >= (int)sc.defs.size() || srel >= (int)sc.defs[stype].members.size())
        return fail(ACL_ERR_FAILED_PRECONDITION, "acl_lookup_resources_multi: unknown subject type or subject relation");
    for (size_t j = 0; j < T; j++) {
        const acl_target_t &t = targets[j];
        if (t.rtype < 0 || t.rtype >= (int)sc.defs.size() || t.permission < 0 || t.permission >= (int)sc.defs[t.rtype].members.size())
            return fail(ACL_ERR_FAILED_PRECONDITION, "acl_lookup_resources_multi: target " + std::to_string(j) + ": unknown type, relation or permission");
    }
    for (size_t j = 0; j < T; j++) {
        const size_t need = ((size_t)h->store.objects(targets[j].rtype).count() + 31) / 32;
        if (row_words[j] < need)
            return fail_detail(ACL_ERR_INVALID_ARGUMENT, kDetailBitmapTooSmall,
                               "acl_lookup_resources_multi: target " + std::to_string(j) + ": bitmap too small (" + std::to_string(need) + " words needed)");
    }
    return ACL_OK;
}

}  // namespace

// n subjects of one class against T targets, rows and counts in the caller's layout (include/aclgpu.h).  Arguments already validated (multi_args_ok).
int lookup_multi(acl_engine *h, PassCtx *c, const acl_target_t *targets, size_t T, int stype, int srel, const uint32_t *sids, size_t n, uint32_t *bitmaps, const size_t *row_words,
                 uint64_t *counts) {
    int rc = not_sharded(h);
    if (rc) return rc;
    if (T == 1) return lookup_batch(h, c, targets[0].rtype, targets[0].permission, stype, srel, sids, n, bitmaps, row_words[0], counts);
    const Schema &sc = h->store.schema();
    const uint32_t key = sc.subject_key(stype, srel < 0 ? kNoRelation : srel);
    MultiTargets mt;
    mt.dev.resize(T);
    mt.off.resize(T);
    std::memset(mt.useful.w, 0, sizeof(mt.useful.w));
    std::memset(mt.is_target.w, 0, sizeof(mt.is_target.w));
    const bool small = h->snap.nslots <= kRevLdsSlots;
    const bool pruned = small && h->rev_sink_on && h->snap.rev_useful.size() >= (size_t)h->snap.nslots * kRevUsefulWords;
    bool fits = true;
    for (size_t j = 0; j < T; j++) {
        const uint32_t slot = (uint32_t)sc.slot(targets[j].rtype, targets[j].permission);
        const size_t need = ((size_t)h->store.objects(targets[j].rtype).count() + 31) / 32;
        if (row_words[j] < need) return fail_detail(ACL_ERR_INVALID_ARGUMENT, kDetailBitmapTooSmall, "lookup: bitmap too small (" + std::to_string(need) + " words needed)");
        // (ids interned since the snapshot was built have no relationship in it: never copy past the slot's id space -- lookup_batch)
        const size_t cw = std::min(need, ((size_t)h->snap.slot_nobjects[slot] + 31) / 32);
        mt.off[j] = mt.stride;
        if (mt.stride > 0xFFFFFFFFull || row_words[j] > 0xFFFFFFFFull) fits = false;
        mt.dev[j] = RevMultiTarget{slot, (uint32_t)mt.stride, (uint32_t)cw, (uint32_t)row_words[j]};
        mt.stride += row_words[j];
        mt.copy_total += cw;
        if (small) {
            mt.is_target.w[slot >> 5] |= 1u << (slot & 31u);
            for (uint32_t k = 0; k < kRevUsefulWords; k++) mt.useful.w[k] |= pruned ? h->snap.rev_useful[(size_t)slot * kRevUsefulWords + k] : 0xFFFFFFFFu;
        }
        if (!h->snap.slot_nonmono.empty() && h->snap.slot_nonmono[slot]) mt.any_nonmono = true;
    }
    // answers subjects [b, b + m) target by target: lookup_batch into rows of its own layout, copied into the caller's
    std::vector<uint32_t> tmp;
    std::vector<uint64_t> tmpc;
    auto per_target = [&](size_t b, size_t m) -> int {
        for (size_t j = 0; j < T; j++) {
            const size_t w = row_words[j];
            tmp.resize(m * std::max<size_t>(w, 1));
            tmpc.resize(m);
            int rc2 = lookup_batch(h, c, targets[j].rtype, targets[j].permission, stype, srel, sids + b, m, tmp.data(), w, tmpc.data());
            if (rc2) return rc2;
            for (size_t i = 0; i < m; i++) {
                if (w) std::memcpy(bitmaps + (b + i) * mt.stride + mt.off[j], tmp.data() + i * w, w * 4);
                if (counts) counts[(b + i) * T + j] = tmpc[i];
            }
        }
        return ACL_OK;
    };
    // The one walk is taken from what the engine can see: k_rev_local itself would be eligible (programs fit its LDS copy, the kernel is on), there are enough
    // targets for it to pay, and their rows are small enough for one block to copy out and clear (acl_engine::rev_multi_min_targets / rev_multi_max_words: both
    // from profiles/lookup_multi_c4.md, DESIGN.md 17 quotes the rows -- beyond the bound the per-target calls, whose big rows live in LDS or go through the
    // chip-wide launches of k_rev_local, are the faster way).
    const size_t vwords = std::max<size_t>((size_t)((h->snap.visited_bits + 31) / 32), 1);
    const DevReverse r0 = h->dev_reverse(c, (uint32_t)vwords);
    const bool multi = fits && h->rev_local && small && r0.nslots <= kRevLdsSlots && r0.nrops <= kRevLdsOps && T >= h->rev_multi_min_targets && mt.copy_total <= h->rev_multi_max_words;
    if (!multi) return per_target(0, n);
    const size_t group = std::max<size_t>(1, std::min<size_t>(n ? n : 1, ((size_t)1 << 28) / vwords));  // <= 1 GiB of visited bits
    for (size_t b = 0; b < n; b += group) {
        const size_t m = std::min(group, n - b);
        rc = check_opts(c->opts);
        if (rc) return rc;
        HIP_TRY(c->visited_zeroed(m * vwords));  // (the kernel takes the rows all zero and hands them back all zero: lookup_batch's contract)
        const DevReverse r = h->dev_reverse(c, (uint32_t)vwords);
        rc = multi_pass_local(h, c, r, key, mt, sids + b, m, bitmaps + b * mt.stride, counts ? counts + b * T : nullptr);
        if (rc == ACL_OK) {
            if (!mt.any_nonmono) continue;
            // targets with `&` / `-` / `.all()`: the walk's rows are candidates, confirmed as the single lookup confirms them
            tmpc.resize(m);
            for (size_t j = 0; j < T; j++) {
                if (!h->snap.slot_nonmono[mt.dev[j].slot]) continue;
                rc = lookup_refine(h, c, targets[j].rtype, targets[j].permission, stype, srel, sids + b, m, bitmaps + b * mt.stride + mt.off[j], mt.stride, mt.dev[j].copy_words, tmpc.data());
                if (rc) return rc;
                for (size_t i = 0; i < m && counts; i++) counts[(b + i) * T + j] = tmpc[i];
            }
            continue;
        }
        c->visited_zero_words = 0;  // a block gave up half-way (or the call failed): its marks are still there
        if (rc != kTakeLevelLoop) return rc;
        rc = per_target(b, m);
        if (rc) return rc;
    }
    return ACL_OK;
}

int lookup_multi_call(acl_engine_t *h, const acl_target_t *targets, size_t T, int stype, int srel, const uint32_t *sids, size_t n, uint32_t *bitmaps, const size_t *row_words,
                      uint64_t *counts, const CallOpts &opts) {
    // arguments first, the engine's mode after them
    if (!T || !n) return ACL_OK;
    if (!targets || !sids || !bitmaps || !row_words) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_lookup_resources_multi: NULL buffer");
    int key_slot = -1;
    {
        std::shared_lock<RwLock> slk(h->state_mu);
        if (!h->store.has_schema()) return fail(ACL_ERR_FAILED_PRECONDITION, "no schema loaded");
        int rc = multi_args_ok(h, targets, T, stype, srel, row_words);
        if (rc) return rc;
        if (srel >= 0) key_slot = h->store.schema().slot(stype, srel);
    }
    Eval ev;
    int rc = ev.begin(h, true, opts, key_slot);
    if (rc) return rc;
    rc = multi_args_ok(h, targets, T, stype, srel, row_words);  // (the schema may have been reloaded in between)
    if (rc) return rc;
    return lookup_multi(h, ev.c, targets, T, stype, srel, sids, n, bitmaps, row_words, counts);
}

// the subject of an access review: strings -> ids, as resolve_lookup does for a LookupResourcesRequest's subject (interned, so `stype:sid#srel` can be its own member)
static int resolve_review_subject(acl_engine_t *h, const char *stype, const char *sid, const char *srel, int *st_out, int *sr_out, uint32_t *sub_out) {
    if (empty(stype) || empty(sid)) return fail(ACL_ERR_INVALID_ARGUMENT, "invalid access review: empty subject field");
    std::shared_lock<RwLock> slk(h->state_mu);
    std::unique_lock<std::shared_mutex> nlk(h->names_mu);
    if (!h->store.has_schema()) return fail(ACL_ERR_FAILED_PRECONDITION, "no schema loaded");
    const Schema &sc = h->store.schema();
    const int st = sc.type_of(stype);
    const bool srel_given = !empty(srel) && std::strcmp(srel, "...") != 0;
    if ((st < 0 && !valid_type_name(stype)) || (srel_given && (st < 0 || sc.defs[st].find(srel) < 0) && !valid_relation_name(srel)) || !valid_object_id(sid))
        return fail(ACL_ERR_INVALID_ARGUMENT, "invalid access review: a subject field does not match the API's pattern");
    if (st < 0) return fail(ACL_ERR_FAILED_PRECONDITION, std::string("object definition `") + stype + "` not found");
    int sr = -1;
    if (srel_given) {
        sr = sc.defs[st].find(srel);
        if (sr < 0) return fail(ACL_ERR_FAILED_PRECONDITION, std::string("relation `") + srel + "` not found under definition `" + stype + "`");
    }
    *sub_out = h->store.intern_object(st, sid);
    *st_out = st;
    *sr_out = sr;
    return ACL_OK;
}

int access_review_call(acl_engine_t *h, const char *stype, const char *sid, const char *srel, const acl_target_t *targets, size_t T, const CallOpts &opts,
                       acl_review_row_t **rows_out, size_t *n_rows_out, uint32_t **bitmaps_out) {
    if (!rows_out || !n_rows_out || !bitmaps_out) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_access_review: NULL output");
    *rows_out = nullptr;
    *n_rows_out = 0;
    *bitmaps_out = nullptr;
    int st, sr;
    uint32_t sub;
    int rc = resolve_review_subject(h, stype, sid, srel, &st, &sr, &sub);
    if (rc) return rc;
    std::vector<acl_target_t> tg;
    {
        std::shared_lock<RwLock> slk(h->state_mu);
        const Schema &sc = h->store.schema();
        if (!targets) {  // every relation and permission of every definition, in slot order
            for (int slot = 0; slot < sc.nslots; slot++) tg.push_back(acl_target_t{(int32_t)sc.slot_owner[slot].first, (int32_t)sc.slot_owner[slot].second});
        } else {
            tg.assign(targets, targets + T);
            for (size_t j = 0; j < T; j++)
                if (tg[j].rtype < 0 || tg[j].rtype >= (int)sc.defs.size() || tg[j].permission < 0 || tg[j].permission >= (int)sc.defs[tg[j].rtype].members.size())
                    return fail(ACL_ERR_FAILED_PRECONDITION, "acl_access_review: target " + std::to_string(j) + ": unknown type, relation or permission");
        }
    }
    T = tg.size();
    acl_review_row_t *rows = (acl_review_row_t *)std::calloc(std::max<size_t>(T, 1), sizeof(acl_review_row_t));
    if (!rows) return fail(ACL_ERR_RESOURCE_EXHAUSTED, "out of host memory for the review's rows");
    std::vector<size_t> words(T);
    std::vector<uint64_t> counts(T);
    rc = owned_bitmap_retry("access review: the object tables kept growing faster than the result bitmaps", [&]() -> int {
        size_t stride = 0;
        for (size_t j = 0; j < T; j++) {
            words[j] = owned_bitmap_words(h, tg[j].rtype);
            rows[j] = acl_review_row_t{tg[j].rtype, tg[j].permission, 0, stride, words[j]};
            stride += words[j];
        }
        uint32_t *bm = nullptr;
        int brc = result_block(stride, "out of host memory for the result bitmaps", &bm);
        if (brc) return brc;
        brc = lookup_multi_call(h, tg.data(), T, st, sr, &sub, 1, bm, words.data(), counts.data(), opts);
        if (brc == ACL_OK) {
            for (size_t j = 0; j < T; j++) rows[j].count = counts[j];
            *rows_out = rows;
            *n_rows_out = T;
            *bitmaps_out = bm;
        } else {
            std::free(bm);
        }
        return brc;
    });
    if (rc) std::free(rows);
    return rc;
}

}  // namespace aclint

using namespace aclint;

extern "C" {

int64_t acl_schema_name_copy(acl_engine_t *h, int type, int member, char *buf, size_t cap) {
    std::shared_lock<RwLock> slk(h->state_mu);
    if (!h->store.has_schema()) return -1;
    const Schema &sc = h->store.schema();
    if (type < 0 || type >= (int)sc.defs.size() || member >= (int)sc.defs[type].members.size()) return -1;
    const std::string &n = member < 0 ? sc.defs[type].name : sc.defs[type].members[member].name;
    if (buf && cap) {
        const size_t k = std::min(n.size(), cap - 1);
        std::memcpy(buf, n.data(), k);
        buf[k] = 0;
    }
    return (int64_t)n.size();
}

int acl_lookup_resources_multi(acl_engine_t *h, const acl_target_t *targets, size_t n_targets, int stype, int srel, const uint32_t *subject_ids, size_t n, uint32_t *bitmaps_out,
                               const size_t *row_words, uint64_t *counts_out, const acl_call_opts_t *o) {
    const CallOpts opts = call_opts(o);
    return lookup_multi_call(h, targets, n_targets, stype, srel, subject_ids, n, bitmaps_out, row_words, counts_out, opts);
}

int acl_access_review(acl_engine_t *h, const char *subject_type, const char *subject_id, const char *subject_relation, const acl_target_t *targets, size_t n_targets,
                      const acl_call_opts_t *o, acl_review_row_t **rows_out, size_t *n_rows_out, uint32_t **bitmaps_out) {
    const CallOpts opts = call_opts(o);
    return access_review_call(h, subject_type, subject_id, subject_relation, targets, n_targets, opts, rows_out, n_rows_out, bitmaps_out);
}
}

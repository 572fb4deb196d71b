// engine_lookup.cpp -- LookupResources: the single-launch reverse walk (k_rev_local), the level loop behind it, the forward
// refinement of candidates under `&` / `-`, and the request's strings -> ids.
#include "engine_internal.hpp"
#include "validate.hpp"

namespace aclint {

// The two halves of a single-launch reverse pass around its launch (RevPass, engine_internal.hpp)
int rev_pass_begin(acl_engine *h, PassCtx *c, size_t m, size_t ncounts, size_t row_bytes, bool may_spin, RevPass *p) {
    uint64_t cap64 = std::min<uint64_t>(c->frontier_entries * 2 / std::max<size_t>(m, 1), 1u << 22);
    if (h->local_cap_limit) cap64 = std::min<uint64_t>(cap64, h->local_cap_limit);
    if (cap64 < 64 || m > 0x7FFFFFFFull) return kTakeLevelLoop;
    p->cap = (uint32_t)cap64;
    p->ncounts = ncounts;
    p->rows_off = 64 + ncounts * sizeof(uint64_t);
    HIP_TRY(c->h_out.ensure(p->rows_off + row_bytes));
    p->flag = (uint32_t *)c->h_out.p;
    p->h_rows = (const uint32_t *)((const char *)c->h_out.p + p->rows_off);
    p->flag[0] = 0;
    p->flag[15] = 0;
    p->d_status = (uint32_t *)c->h_out.dp;
    p->d_counts = (uint64_t *)((char *)c->h_out.dp + 64);
    p->d_rows = (uint32_t *)((char *)c->h_out.dp + p->rows_off);
    p->spin = may_spin && m <= h->spin_max && !c->timing;
    p->done_val = p->spin ? next_done_val(c) : 0u;
    p->d_done_flag = p->spin ? p->d_status + 15 : nullptr;
    return ACL_OK;
}

int rev_pass_end(PassCtx *c, const RevPass &p, uint64_t *counts) {
    // (the proxy's shape is ONE LookupResources per list request, lookups.go:65: the caller spins on the completion word -- spin_for)
    if (!(p.spin && spin_for(p.flag + 15, p.done_val))) HIP_TRY(hipStreamSynchronize(c->stream));
    ev_collect(c);
    if (*p.flag == 2) return fail(ACL_ERR_RESOURCE_EXHAUSTED, "a relationship row exceeds the per-task enumeration limit");
    if (*p.flag) {
        c->stats.overflow_retries++;
        return kTakeLevelLoop;
    }
    const uint64_t *h_counts = (const uint64_t *)((const char *)c->h_out.p + 64);
    uint32_t levels = 0;
    for (size_t k = 0; k < p.ncounts; k++) {  // count | levels walked << 56
        levels = std::max<uint32_t>(levels, (uint32_t)(h_counts[k] >> 56));
        if (counts) counts[k] = h_counts[k] & 0x00FFFFFFFFFFFFFFull;
    }
    c->stats.levels_last = levels;
    return ACL_OK;
}

// Single-launch LookupResources over m subjects already staged in c->h_in (pinned).  Result rows go to `bitmaps` directly when the
// caller's buffer is pinned (acl_host_alloc), else through the context's pinned staging.  kTakeLevelLoop: a block outgrew its share.
// d_dst != NULL (watch sets, engine_watchset.cpp): the rows stay on the device, row i at d_dst + i * dstride (dstride >= cw words, the words behind cw
// zeroed); `bitmaps` is not touched.
static int lookup_pass_local(acl_engine *h, PassCtx *c, const DevReverse &r, uint32_t key, uint32_t target, size_t m, uint32_t *bitmaps, size_t words, size_t cw,
                             uint64_t *counts, uint32_t *d_dst = nullptr, size_t dstride = 0) {
    if (words > 0xFFFFFFFFull || r.nslots > kRevLdsSlots || r.nrops > kRevLdsOps) return kTakeLevelLoop;
    const bool direct = !d_dst && words && h->is_pinned(bitmaps, m * words * sizeof(uint32_t));
    const size_t ostride = d_dst ? dstride : direct ? words : cw;
    // Result rows: written by the kernel straight into host memory (each block as it finishes)
    RevPass p;
    int rc = rev_pass_begin(h, c, m, m, (direct || d_dst) ? 0 : m * std::max<size_t>(cw, 1) * 4, !d_dst, &p);
    if (rc) return rc;
    void *d_rows = p.d_rows;
    if (d_dst) d_rows = d_dst;
    else if (direct) HIP_TRY(hipHostGetDevicePointer(&d_rows, bitmaps, 0));
    // Rows that do not fit the block's LDS (a type of more than 1 M objects; reference pkg/authz/lookups.go:49-65 asks for the whole type): the heavy terminal
    // rows are deferred to a chip-wide launch and the rows are copied / counted / cleared by a third one (kernels.hip RevDefer; ACL_REV_BIG_ROWS=0: one block
    // does it all, as in round 5 -- A/B)
    const uint32_t lds_row_words = h->rev_lds_rows ? (uint32_t)(((size_t)h->snap.slot_nobjects[target] + 31) / 32) : 0u;
    RevBigRows big;
    const size_t bm_stride = (((size_t)h->snap.slot_nobjects[target] + 127) / 128) * 128;
    // (a result slot that is a sink of the reverse graph is marked, not expanded: Snapshot::rev_sink; ACL_REV_SINK=0 at acl_open: A/B and test knob)
    const bool sink = h->rev_sink_on && h->shard.world == 1 && target < h->snap.rev_sink.size() && h->snap.rev_sink[target];
    const bool use_big = h->rev_big_rows && (lds_row_words == 0 || (size_t)lds_row_words * 4 > kRevLdsRowBytes) && cw > 0 &&
                         ((h->snap.rprogs[target].n & ~kRevRemoteBit) == 0 || sink) &&  // (a result slot nobody expands: its marks need no first-visit answer)
                         m * bm_stride <= ((size_t)2 << 30) && bm_stride <= 0xFFFFFF80ull;
    if (use_big) {
        if (c->d_big_bytes.n < m * bm_stride || !c->d_big_bytes.p) {
            HIP_TRY(c->d_big_bytes.ensure(m * bm_stride));
            c->big_bytes_zeroed = 0;
        }
        if (c->big_bytes_zeroed < m * bm_stride) {
            HIP_TRY(hipMemsetAsync(c->d_big_bytes.p, 0, m * bm_stride, c->stream));
            c->big_bytes_zeroed = m * bm_stride;
        }
        const size_t tcap = std::min<size_t>(1u << 16, std::max<size_t>(4096, ((size_t)64 << 20) / 8 / m));  // <= 64 MiB of task lists per batch
        HIP_TRY(c->d_big_tasks.ensure(m * tcap));
        HIP_TRY(c->d_big_meta.ensure(2 * m));
        if (c->d_big_counts.n < m || !c->d_big_counts.p) {
            HIP_TRY(c->d_big_counts.ensure(m));
            c->big_counts_zeroed = 0;
        }
        if (c->big_counts_zeroed < m) {
            HIP_TRY(hipMemsetAsync(c->d_big_counts.p, 0, m * sizeof(uint64_t), c->stream));
            c->big_counts_zeroed = m;
        }
        HIP_TRY(c->d_done.ensure(1));
        big = RevBigRows{c->d_big_bytes.p, (uint32_t)bm_stride, c->d_big_tasks.p, c->d_big_meta.p, c->d_big_meta.p + m, c->d_big_counts.p, (uint32_t)tcap, h->rev_defer_min};
    }
    ev_begin(c, 3);
    RevUseful useful;  // (the slots that can lead to the result slot: everything else is dead weight for this lookup)
    const bool pruned = h->rev_sink_on && h->shard.world == 1 && h->snap.rev_useful.size() >= ((size_t)target + 1) * kRevUsefulWords;
    if (pruned) std::memcpy(useful.w, h->snap.rev_useful.data() + (size_t)target * kRevUsefulWords, sizeof(useful.w));
    launch_rev_local(c->stream, r, (const uint32_t *)c->h_in.dp, (uint32_t)m, key, target | (sink ? kRevTargetSink : 0u), c->d_fbuf[0].p, p.cap, (uint32_t *)d_rows, (uint32_t)ostride,
                     (uint32_t)cw, p.d_counts, p.d_status, lds_row_words, (p.spin || use_big) ? c->d_done.p : nullptr, p.d_done_flag, p.done_val, use_big ? &big : nullptr,
                     pruned ? &useful : nullptr);
    ev_end(c);
    rc = rev_pass_end(c, p, counts);
    const uint32_t *flag = p.flag;
    if (*flag && use_big) c->big_bytes_zeroed = 0;  // (a block gave up half-way: marks of rows nobody folded may be left)
    static const bool kDebugRev = getenv("ACL_DEBUG_REV") != nullptr;  // (stderr: what the walk deferred -- tools/lookup_big_probe.py)
    if (kDebugRev && use_big) {
        std::vector<uint32_t> meta(2 * m);
        std::vector<uint64_t> tk(std::min<size_t>(big.task_cap, 4096));
        (void)hipMemcpy(meta.data(), c->d_big_meta.p, meta.size() * 4, hipMemcpyDeviceToHost);
        for (size_t i = 0; i < std::min<size_t>(m, 4); i++) {
            (void)hipMemcpy(tk.data(), c->d_big_tasks.p + i * big.task_cap, std::min<size_t>(meta[i], tk.size()) * 8, hipMemcpyDeviceToHost);
            uint64_t kids = 0;
            for (size_t k = 0; k < std::min<size_t>(meta[i], tk.size()); k++) kids += tk[k] >> 32;
            fprintf(stderr, "[aclgpu] lookup %zu: %u deferred rows (%llu children in the first %zu), %u reverse levels, status %u\n", i, meta[i], (unsigned long long)kids,
                    std::min<size_t>(meta[i], tk.size()), meta[m + i], *flag);
        }
    }
    if (rc) return rc;
    for (size_t i = 0; i < m && !direct && !d_dst; i++) {
        uint32_t *dst = bitmaps + i * words;
        if (cw) std::memcpy(dst, p.h_rows + i * cw, cw * 4);
        std::fill(dst + cw, dst + words, 0u);
    }
    c->stats.rev_local_passes++;
    c->stats.lookup_requests += m;
    return ACL_OK;
}

// Schemas with `&` / `-`: the reverse walk only follows POSITIVE occurrences (plan_reverse.cpp), so what it marks is a superset -- the
// candidates.  The answer is the candidates the forward walk grants: one bulk Check per lookup batch, bits of everything but HAS cleared.
// (LookupResources(T, p, S) = {id : Check(T:id#p@S) = HAS}; reference call site pkg/authz/lookups.go:65.)
// A candidate whose Check ERRS (a branch beyond the dispatch depth under an `&` / `-`) fails the CALL with that item's code: the reference's
// stream ends at the first Recv error (lookups.go:75-83) and the list request with it (responsefilterer.go:196-204) -- it never sees a
// silently shorter list.  ACL_FLAG_LENIENT_LOOKUP keeps the round-4/5 behaviour (such candidates are dropped, the call succeeds).
int lookup_candidate_error(acl_engine *h, int32_t code, uint32_t id, uint32_t sid) {
    (void)h;
    return fail(code, std::string(code == ACL_ERR_DEPTH ? "LookupResources: max depth exceeded" : "LookupResources: a candidate's check failed") + " while checking candidate id " +
                          std::to_string(id) + " for subject id " + std::to_string(sid) + " (the permission holds an intersection / exclusion: candidates are confirmed by a forward Check)");
}
int lookup_refine(acl_engine *h, PassCtx *c, int rtype, int perm, int stype, int srel, const uint32_t *sids, size_t n, uint32_t *bitmaps, size_t words, size_t cw,
                  uint64_t *counts) {
    std::vector<acl_item_t> items;
    std::vector<uint8_t> answers;
    std::vector<int32_t> errs;
    const uint16_t sr = (uint16_t)(srel < 0 ? ACL_NO_RELATION : srel);
    const size_t chunk = std::max<size_t>(h->max_sub_batch, 1);
    const bool strict = !h->lenient_lookup;
    size_t i0 = 0;  // first lookup whose candidates are in `items`
    auto flush = [&](size_t i1) -> int {  // answers the candidates of lookups [i0, i1) and clears the denied ones
        if (!items.empty()) {
            answers.resize(items.size());
            if (strict) errs.assign(items.size(), 0);
            for (size_t b = 0; b < items.size(); b += chunk) {
                int rc = check_ids_host(h, c, items.data() + b, std::min(chunk, items.size() - b), answers.data() + b, strict ? errs.data() + b : nullptr);
                if (rc) return rc;
            }
            if (strict)
                for (size_t k = 0; k < items.size(); k++)
                    if (errs[k]) return lookup_candidate_error(h, errs[k], items[k].resource_id, items[k].subject_id);
            size_t k = 0;
            for (size_t i = i0; i < i1; i++) {
                uint32_t *row = bitmaps + i * words;
                for (size_t w = 0; w < cw; w++)
                    for (uint32_t m = row[w]; m; m &= m - 1, k++)
                        if (answers[k] != ACL_PERM_HAS_PERMISSION) row[w] &= ~(m & (0u - m));
            }
        }
        for (size_t i = i0; i < i1; i++)
            if (counts) counts[i] = popcount_words(bitmaps + i * words, cw);
        items.clear();
        i0 = i1;
        return ACL_OK;
    };
    for (size_t i = 0; i < n; i++) {
        const uint32_t *row = bitmaps + i * words;
        for (size_t w = 0; w < cw; w++)
            for (uint32_t m = row[w]; m; m &= m - 1)
                items.push_back(acl_item_t{(uint16_t)rtype, (uint16_t)perm, (uint32_t)(w * 32 + (size_t)__builtin_ctz(m)), (uint16_t)stype, sr, sids[i]});
        if (items.size() >= chunk)
            if (int rc = flush(i + 1)) return rc;
    }
    return flush(n);
}

// one batched reverse walk: n subjects of one class against one (type, permission); bitmaps in host memory -- or, with d_dst, left on the device
// (row i at d_dst + i * dstride, dstride >= the words the type's ids need, zero behind them; `bitmaps`, `words` and `counts` are not used, and the
// permission must be monotone: candidates under `&` / `-` are confirmed on host rows)
int lookup_batch(acl_engine *h, PassCtx *c, int rtype, int perm, int stype, int srel, const uint32_t *sids, size_t n, uint32_t *bitmaps, size_t words,
                 uint64_t *counts, uint32_t *d_dst, size_t dstride) {
    int rc = not_sharded(h);
    if (rc) return rc;
    const Schema &sc = h->store.schema();
    const uint32_t target = (uint32_t)sc.slot(rtype, perm);
    const uint32_t key = sc.subject_key(stype, srel < 0 ? kNoRelation : srel);
    const uint32_t nobj = h->store.objects(rtype).count();
    const size_t need = (nobj + 31) / 32;
    if (d_dst) {
        if (dstride < need || (!h->snap.slot_nonmono.empty() && h->snap.slot_nonmono[target])) return fail(ACL_ERR_INTERNAL, "lookup: device rows too narrow, or asked for a permission with `&` / `-`");
        words = dstride;
        counts = nullptr;
    }
    if (words < need) return fail_detail(ACL_ERR_INVALID_ARGUMENT, kDetailBitmapTooSmall, "lookup: bitmap too small (" + std::to_string(need) + " words needed)");
    // the walk can only mark the ids the snapshot's bitmap slot covers (the build-time count plus headroom); ids interned
    // since then have no relationship in this snapshot, so their bits are zero -- never copy past the slot (advice r1)
    const size_t slot_words = ((size_t)h->snap.slot_nobjects[target] + 31) / 32;
    const size_t cw = std::min(need, slot_words);
    const size_t vwords = std::max<size_t>((size_t)((h->snap.visited_bits + 31) / 32), 1);
    const size_t group = std::max<size_t>(1, std::min<size_t>(n ? n : 1, ((size_t)1 << 28) / vwords));  // <= 1 GiB of visited bits
    for (size_t b = 0; b < n; b += group) {
        const size_t m = std::min(group, n - b);
        // (the single-launch walk takes the visited rows all zero and leaves them all zero -- every block clears what it marked; the level loop zeroes them itself)
        HIP_TRY(h->rev_local ? c->visited_zeroed(m * vwords) : c->d_visited.ensure(m * vwords));
        HIP_TRY(c->d_sids.ensure(m));
        HIP_TRY(c->h_in.ensure(m * sizeof(uint32_t)));
        std::memcpy(c->h_in.p, sids + b, m * sizeof(uint32_t));
        DevReverse r = h->dev_reverse(c, (uint32_t)vwords);
        // ONE launch for the whole group (k_rev_local: a block per lookup walks every reverse level, marks the result bits where they are
        // produced, and writes the result rows + id counts straight into host memory): no per-level launches, no status round trips, no
        // memset, no D2H copies.  A lookup that outgrows its block (private frontier region, children per level) sends the group to the
        // level loop below, which spreads it over the chip.
        if (h->rev_local) {
            rc = lookup_pass_local(h, c, r, key, target, m, d_dst ? nullptr : bitmaps + b * words, words, cw, counts ? counts + b : nullptr, d_dst ? d_dst + b * dstride : nullptr,
                                   dstride);
            if (rc == ACL_OK) continue;
            c->visited_zero_words = 0;  // a block gave up half-way (or the call failed): its marks are still there
            if (rc != kTakeLevelLoop) return rc;
        }
        c->visited_zero_words = 0;  // (the level loop below marks and does not clear)
        HIP_TRY(hipMemcpyAsync(c->d_sids.p, c->h_in.p, m * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        if (d_dst) HIP_TRY(hipMemsetAsync(d_dst + b * dstride, 0, m * dstride * 4, c->stream));  // (the copy below brings cw words per row)
        else HIP_TRY(c->h_out.ensure(m * std::max<size_t>(cw, 1) * 4));
        for (int attempt = 0;; attempt++) {
            if (m > c->frontier_entries) {
                rc = alloc_frontier(h, c, m * 4);
                if (rc) return rc;
            }
            DevFrontier f = h->dev_frontier(*c);
            HIP_TRY(hipMemsetAsync(c->d_visited.p, 0, m * vwords * 4, c->stream));
            launch_rev_seed(c->stream, f, c->d_sids.p, (uint32_t)m, key);  // seeds + status block, on the device
            DevReverse rl = r;  // (the level loop walks towards the result slot too: dead ops skipped -- not on a sharded graph, whose programs are one shard's)
            if (h->rev_sink_on && h->shard.world == 1 && h->snap.rev_useful.size() >= ((size_t)target + 1) * kRevUsefulWords)
                std::memcpy(rl.useful, h->snap.rev_useful.data() + (size_t)target * kRevUsefulWords, sizeof(rl.useful));
            uint32_t levels = 0;
            hipError_t cpe = hipSuccess;
            rc = level_loop(h, c, kMaxLevels + 1, [&](uint32_t it) { launch_rev_expand(c->stream, rl, f, it); }, &levels, [&] {
                // speculative epilogue: the result rows of the target slot, one strided copy for all requests
                if (cw) {
                    hipError_t e = d_dst ? hipMemcpy2DAsync(d_dst + b * dstride, dstride * 4, c->d_visited.p + h->snap.slot_bit_base[target] / 32, vwords * 4, cw * 4, m,
                                                            hipMemcpyDeviceToDevice, c->stream)
                                         : hipMemcpy2DAsync(c->h_out.p, cw * 4, c->d_visited.p + h->snap.slot_bit_base[target] / 32, vwords * 4, cw * 4, m,
                                                            hipMemcpyDeviceToHost, c->stream);
                    if (e != hipSuccess) cpe = e;
                }
            });
            if (rc == ACL_ERR_RESOURCE_EXHAUSTED && c->h_status[2 * kLevelSlots] == 1) {
                c->stats.overflow_retries++;
                if (c->frontier_entries >= (uint64_t)kMaxFrontierChunks * kChunk || attempt > 8) return fail(ACL_ERR_RESOURCE_EXHAUSTED, "frontier capacity exceeded in lookup");
                int rc2 = alloc_frontier(h, c, c->frontier_entries * 4);
                if (rc2) return rc2;
                continue;
            }
            if (rc) return rc;
            if (cpe != hipSuccess) return fail(ACL_ERR_INTERNAL, std::string("lookup result copy: ") + hipGetErrorString(cpe));
            break;
        }
        c->stats.lookup_requests += m;
        for (size_t i = 0; i < m && !d_dst; i++) {
            uint32_t *dst = bitmaps + (b + i) * words;
            if (cw) std::memcpy(dst, (const uint32_t *)c->h_out.p + i * cw, cw * 4);
            std::fill(dst + cw, dst + words, 0u);
            if (counts) counts[b + i] = popcount_words(dst, cw);
        }
    }
    if (!d_dst && !h->snap.slot_nonmono.empty() && h->snap.slot_nonmono[target]) return lookup_refine(h, c, rtype, perm, stype, srel, sids, n, bitmaps, words, cw, counts);
    return ACL_OK;
}

// LookupResourcesRequest strings -> ids (lookups.go:49-62); the subject is interned so `stype:sid#srel` can be its own member
int resolve_lookup(acl_engine_t *h, const char *rtype, const char *perm, const char *stype, const char *sid, const char *srel, int *rt_out, int *pm_out,
                   int *st_out, int *sr_out, uint32_t *sub_out) {
    if (empty(rtype) || empty(perm) || empty(stype) || empty(sid)) return fail(ACL_ERR_INVALID_ARGUMENT, "invalid LookupResourcesRequest: empty field");
    std::shared_lock<RwLock> slk(h->state_mu);
    std::unique_lock<std::shared_mutex> nlk(h->names_mu);
    if (!h->store.has_schema()) return fail(ACL_ERR_FAILED_PRECONDITION, "no schema loaded");
    const Schema &sc = h->store.schema();
    int sr = -1;
    const int rt = sc.type_of(rtype);
    {   // API validation first (validate.hpp)
        const int vs = sc.type_of(stype);
        const bool srel_given = !empty(srel) && std::strcmp(srel, "...") != 0;
        if ((rt < 0 && !valid_type_name(rtype)) || (vs < 0 && !valid_type_name(stype)) || ((rt < 0 || sc.defs[rt].find(perm) < 0) && !valid_relation_name(perm)) ||
            (srel_given && (vs < 0 || sc.defs[vs].find(srel) < 0) && !valid_relation_name(srel)) || !valid_object_id(sid))
            return fail(ACL_ERR_INVALID_ARGUMENT, "invalid LookupResourcesRequest: a field does not match the API's pattern");  // (`*` is not an object id here)
    }
    if (rt < 0) return fail(ACL_ERR_FAILED_PRECONDITION, std::string("object definition `") + rtype + "` not found");
    const int pm = sc.defs[rt].find(perm);
    if (pm < 0) return fail(ACL_ERR_FAILED_PRECONDITION, std::string("relation/permission `") + perm + "` not found under definition `" + rtype + "`");
    const int st = sc.type_of(stype);
    if (st < 0) return fail(ACL_ERR_FAILED_PRECONDITION, std::string("object definition `") + stype + "` not found");
    if (!empty(srel) && std::strcmp(srel, "...") != 0) {
        sr = sc.defs[st].find(srel);
        if (sr < 0) return fail(ACL_ERR_FAILED_PRECONDITION, std::string("relation `") + srel + "` not found under definition `" + stype + "`");
    }
    *sub_out = h->store.intern_object(st, sid);  // (a subject nobody has a relationship with: reusable after the quarantine, store.hpp)
    *rt_out = rt;
    *pm_out = pm;
    *st_out = st;
    *sr_out = sr;
    return ACL_OK;
}

static int lookup_args_ok(acl_engine *h, int rtype, int perm, int stype, int srel) {
    const Schema &sc = h->store.schema();
    if (rtype < 0 || rtype >= (int)sc.defs.size() || stype < 0 || stype >= (int)sc.defs.size() || perm < 0 ||
        perm >= (int)sc.defs[rtype].members.size() || srel >= (int)sc.defs[stype].members.size())
        return fail(ACL_ERR_FAILED_PRECONDITION, "lookup: unknown type, permission or subject relation");
    return ACL_OK;
}

int lookup_batch_call(acl_engine_t *h, int rtype, int perm, int stype, int srel, const uint32_t *sids, size_t n, uint32_t *bitmaps, size_t words,
                             uint64_t *counts, const CallOpts &opts) {
    if (n && (!sids || !bitmaps)) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_lookup_resources_batch: NULL buffer");
    int key_slot = -1;
    {
        std::shared_lock<RwLock> slk(h->state_mu);
        if (!h->store_only) {
            if (!h->store.has_schema()) return fail(ACL_ERR_FAILED_PRECONDITION, "no schema loaded");
            int rc = lookup_args_ok(h, rtype, perm, stype, srel);
            if (rc) return rc;
            if (srel >= 0) key_slot = h->store.schema().slot(stype, srel);
        }
    }
    Eval ev;
    int rc = ev.begin(h, true, opts, key_slot);
    if (rc) return rc;
    rc = lookup_args_ok(h, rtype, perm, stype, srel);  // (the schema may have been reloaded in between)
    if (rc) return rc;
    return lookup_batch(h, ev.c, rtype, perm, stype, srel, sids, n, bitmaps, words, counts);
}

int lookup_opts_call(acl_engine_t *h, const char *rtype, const char *perm, const char *stype, const char *sid, const char *srel, uint32_t *bitmap_out,
                     size_t bitmap_words, uint64_t *count_out, const CallOpts &opts) {
    int rt, pm, st, sr;
    uint32_t sub;
    int rc = resolve_lookup(h, rtype, perm, stype, sid, srel, &rt, &pm, &st, &sr, &sub);
    if (rc) return rc;
    return lookup_batch_call(h, rt, pm, st, sr, &sub, 1, bitmap_out, bitmap_words, count_out, opts);
}

}  // namespace aclint

// engine_shard_subjects.cpp -- LookupSubjects on the type-hash sharded graph: the native level loop (acl_shard_subjects_bulk).
//
// The unsharded walk (kernels.hip k_subj_local) is one block's private log and needs every row it can reach in that device's HBM.  Here the walk is
// level-synchronous and chip-wide (k_subj_expand): a state is expanded on the shard that owns its slot's type, over that shard's subject rows (the
// transpose of the classes it holds: plan_subjects.cpp), and a child of another shard's type crosses in the level's exchange -- the same Exchange, the
// same communicator callbacks and the same cycle, Exchange::walk (engine_shard_exchange.hpp), as the Check and LookupResources loops (engine_shard_native.cpp).
//   * visited bits live on the owner only; every visit decision for level L is taken during iteration L - 1 (kernels.hip, above k_subj_expand);
//   * every shard marks the subjects ITS rows name into a partial row; the partial rows are all-gathered and OR-ed (k_subj_fold) -- not max-reduced
//     byte-wise: several shards set different bits of one byte.  Wildcard flags are one 0/1 byte per lookup: those are max-reduced;
//   * the lookups are cut into chunks so that visited bits, partial rows and the gathered rows stay bounded; the chunk size depends only on what every
//     rank shares (schema, object counts, world), so the collectives stay in lockstep;
//   * a permission with `-`, `&` or `.all()` is walked by its positive relaxation; every shard then holds the same candidate rows, builds the same
//     items and takes part in ONE sharded Check per slice (shard_check_core), exactly as acl_shard_lookup_bulk confirms its candidates.
// Afterwards every shard holds the same rows, flags and excluded rows; a failure is taken by all shards or by none.
#include "engine_shard_exchange.hpp"

namespace {

constexpr size_t kSubjChunkWords = (size_t)1 << 28;  // <= 1 GiB of visited bits + partial rows per chunk (engine_subjects.cpp subjects_walk), and of gathered rows

}  // namespace

extern "C" {

int acl_shard_subjects_bulk(acl_engine_t *h, const acl_shard_comm_t *comm, int rtype, int perm, int stype, int srel, const uint32_t *rids, size_t n, void *d_bitmaps_out,
                            size_t bitmap_words, uint8_t *flags_out, void *d_excluded_out, acl_shard_bulk_stats_t *stats_out) {
    if (!comm || !comm->all_gather || !comm->all_reduce_max_u8) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_shard_subjects_bulk: communicator callbacks missing");
    if (n && (!rids || !d_bitmaps_out)) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_shard_subjects_bulk: NULL buffer");
    if (n > 0xFFFFFFF0ull) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_shard_subjects_bulk: batch too large");
    ShardCall scall;
    int rc = scall.begin(h, true, false, true, true);
    if (rc) return rc;
    PassCtx *c = scall.c;
    if (!h->store.has_schema()) return fail(ACL_ERR_FAILED_PRECONDITION, "no schema loaded");
    const Schema &sc = h->store.schema();
    if (rtype < 0 || rtype >= (int)sc.defs.size() || stype < 0 || stype >= (int)sc.defs.size() || perm < 0 || perm >= (int)sc.defs[rtype].members.size() ||
        srel >= (int)sc.defs[stype].members.size())
        return fail(ACL_ERR_FAILED_PRECONDITION, "lookup_subjects: unknown type, permission or subject relation");
    const uint32_t target = (uint32_t)sc.slot(rtype, perm);
    const uint32_t key = sc.subject_key(stype, srel < 0 ? kNoRelation : srel);
    const uint32_t nobj = h->store.objects(stype).count();
    const size_t need = ((size_t)nobj + 31) / 32;
    if (n && bitmap_words < need) return fail(ACL_ERR_INVALID_ARGUMENT, "lookup_subjects: bitmap too small (" + std::to_string(need) + " words needed)");
    const uint32_t nres = h->store.objects(rtype).count();
    for (size_t i = 0; i < n; i++)
        if (rids[i] >= nres) return fail(ACL_ERR_INVALID_ARGUMENT, "lookup_subjects: resource id " + std::to_string(rids[i]) + " beyond the type's objects");
    const uint32_t world = h->shard.world;
    const SubjectRows &sr = h->subj;
    const DevSubjects g = dev_subjects(h, c);
    const size_t vwords = sr.visited_words;
    // lookups per chunk, from what every rank shares: the visited words if EVERY slot had bits for its type's objects as they are now (a bound of this
    // shard's own vwords, whenever its rows were built), the row words, the world
    size_t vbound = 0;
    for (int slot = 0; slot < sc.nslots; slot++) vbound += ((size_t)with_headroom(h->store.objects(sc.slot_owner[slot].first).count()) + 31) / 32;
    size_t mmax = std::max<size_t>(1, kSubjChunkWords / std::max<size_t>(vbound + need, 1));
    mmax = std::min(mmax, std::max<size_t>(1, kSubjChunkWords / std::max<size_t>((size_t)world * need, 1)));
    acl_shard_bulk_stats_t st{};
    Exchange X{h, c, comm, world, h->shard.rank, 0, comm->all_to_all != nullptr && world <= kMaxShards && h->shard_a2a, &st, &c->xplan_subj};
    first_xcap(c);
    HIP_TRY(c->d_subj_flags.ensure((std::max<size_t>(n, 1) + 3) / 4));
    uint8_t *d_flags = reinterpret_cast<uint8_t *>(c->d_subj_flags.p);
    for (size_t b = 0; b < n;) {
        const size_t m = std::min(n - b, mmax);
        if (m > c->frontier_entries) {
            rc = alloc_frontier(h, c, m * 4);
            if (rc) return rc;
        }
        HIP_TRY(c->d_sids.ensure(m));
        HIP_TRY(c->d_subj_visited.ensure(m * vwords));
        HIP_TRY(c->d_subj_rows.ensure(std::max<size_t>(m * need, 1)));
        HIP_TRY(c->h_in.ensure(m * sizeof(uint32_t)));
        std::memcpy(c->h_in.p, rids + b, m * sizeof(uint32_t));
        HIP_TRY(hipMemcpyAsync(c->d_sids.p, c->h_in.p, m * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        DevFrontier f;
        DevShard sh;
        DevSubjLevel s;
        uint32_t done_at = 0;
        rc = X.walk(
            WalkShape{1, 1, kMaxLevels, std::max<uint32_t>(c->subj_levels_hint, 2), 4},
            [&]() -> int {
                f = h->dev_frontier(*c);
                sh = X.shard();
                s = DevSubjLevel{g, c->d_subj_visited.p, c->d_subj_rows.p, d_flags + b, (uint32_t)need, key};
                HIP_TRY(hipMemsetAsync(c->d_subj_visited.p, 0, m * vwords * 4, c->stream));
                if (need) HIP_TRY(hipMemsetAsync(c->d_subj_rows.p, 0, m * need * 4, c->stream));
                HIP_TRY(hipMemsetAsync(d_flags + b, 0, m, c->stream));
                ev_begin(c, 0);
                launch_subj_seed(c->stream, s, f, c->d_sids.p, (uint32_t)m, target, sh);  // seeds + status block
                ev_end(c);
                return ACL_OK;
            },
            [&](uint32_t it) -> int {
                ev_begin(c, 1);
                launch_subj_expand(c->stream, s, f, it, sh);
                ev_end(c);
                int rc = X.run(it, [&](const uint4 *hdrs, const uint4 *data, bool have, uint32_t *ctrl) {
                    launch_subj_import_gathered(c->stream, s, f, it, hdrs, data, X.world, X.rank, X.cap, have, ctrl);
                });
                if (rc) return rc;
                c->stats.expand_launches++;
                return ACL_OK;
            },
            [](uint32_t, uint32_t, int) { return 0; }, &done_at);
        if (rc) return rc;
        c->subj_levels_hint = done_at;
        st.levels = std::max(st.levels, done_at);
        // result rows: every shard marked what ITS rows name; gathered and OR-ed, the same on every shard
        uint32_t *out = reinterpret_cast<uint32_t *>(d_bitmaps_out) + b * bitmap_words;
        if (need) {
            HIP_TRY(c->d_rows.ensure((size_t)world * m * need));
            rc = comm->all_gather(comm->user, c->d_subj_rows.p, c->d_rows.p, m * need * 4, (void *)c->stream);
            if (rc) return rc;
            st.exchanged_bytes += (uint64_t)world * m * need * 4;
            launch_subj_fold(c->stream, c->d_rows.p, world, (uint32_t)m, (uint32_t)need, out, (uint32_t)bitmap_words);
        } else if (bitmap_words) {
            HIP_TRY(hipMemsetAsync(out, 0, m * bitmap_words * 4, c->stream));
        }
        b += m;
    }
    std::vector<uint8_t> wild(n, 0);
    if (n) {
        rc = comm->all_reduce_max_u8(comm->user, d_flags, n, (void *)c->stream);  // (one 0/1 byte per lookup: a max is an OR)
        if (rc) return rc;
        HIP_TRY(c->h_out.ensure(n));
        HIP_TRY(hipMemcpyAsync(c->h_out.p, d_flags, n, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    ev_collect(c);
    st.host_syncs++;
    if (n) std::memcpy(wild.data(), c->h_out.p, n);
    st.export_capacity = X.cap ? X.cap : c->xcap;
    // ---- a permission that can depend on `-`, `&` or `.all()`: the rows are candidates.  Every shard holds the same rows by now, builds the same items (+ the
    // wildcard's stand-in: a subject nobody names) and takes part in one sharded Check per bounded slice of lookups -- the collectives stay in lockstep.
    const bool nonmono = h->snap.slot_nonmono.size() > target && h->snap.slot_nonmono[target];
    const bool strict = !h->lenient_lookup;
    const uint16_t srl = (uint16_t)(srel < 0 ? ACL_NO_RELATION : srel);
    std::vector<acl_item_t> items;
    std::vector<uint8_t> ans;
    std::vector<int32_t> err;
    acl_shard_bulk_stats_t cst{};
    if (n && nonmono) {
        std::vector<uint32_t> rows(n * bitmap_words);
        if (!rows.empty()) HIP_TRY(hipMemcpy(rows.data(), d_bitmaps_out, rows.size() * 4, hipMemcpyDeviceToHost));
        const size_t limit = std::max<size_t>(h->max_sub_batch, 1);
        size_t i0 = 0;
        while (i0 < n) {
            items.clear();
            size_t i1 = i0;
            for (; i1 < n && (i1 == i0 || items.size() < limit); i1++) {
                const uint32_t *row = rows.data() + i1 * bitmap_words;
                for (size_t w = 0; w < need; w++)
                    for (uint32_t mm = row[w]; mm; mm &= mm - 1)
                        items.push_back(acl_item_t{(uint16_t)rtype, (uint16_t)perm, rids[i1], (uint16_t)stype, srl, (uint32_t)(w * 32 + (size_t)__builtin_ctz(mm))});
                if (wild[i1]) items.push_back(acl_item_t{(uint16_t)rtype, (uint16_t)perm, rids[i1], (uint16_t)stype, srl, kFreshSubject});
            }
            rc = check_candidates(h, c, comm, items, &ans, &err, &cst);
            if (rc) return rc;
            add_stats(&st, cst);
            size_t k = 0;
            for (size_t i = i0; i < i1; i++) {  // (every shard holds the same answers: all of them fail, or none)
                uint32_t *row = rows.data() + i * bitmap_words;
                for (size_t w = 0; w < need; w++)
                    for (uint32_t mm = row[w]; mm; mm &= mm - 1, k++) {
                        if (err[k] && strict) return subjects_error(err[k], rids[i], items[k].subject_id);
                        if (err[k] || ans[k] != ACL_PERM_HAS_PERMISSION) row[w] &= ~(mm & (0u - mm));
                    }
                if (wild[i]) {
                    if (err[k] && strict) return subjects_error(err[k], rids[i], kFreshSubject);
                    wild[i] = !err[k] && ans[k] == ACL_PERM_HAS_PERMISSION;
                    k++;
                }
            }
            i0 = i1;
        }
        if (!rows.empty()) HIP_TRY(hipMemcpy(d_bitmaps_out, rows.data(), rows.size() * 4, hipMemcpyHostToDevice));
    }
    // ---- excluded: who of the whole subject type does NOT hold the permission, for the lookups a confirmed wildcard answers (a monotone permission
    // that a wildcard grants excludes nobody).  The wildcard's own id (the name "*") is not a subject.
    if (d_excluded_out && n && bitmap_words) {
        std::vector<uint32_t> ex(n * bitmap_words, 0u);
        for (size_t i = 0; i < n && nonmono; i++) {
            if (!wild[i]) continue;
            const uint32_t wid = h->store.wildcard_id(stype);
            const size_t chunk = std::min<size_t>(std::max<size_t>(h->max_sub_batch, 1), 262144);
            for (size_t s0 = 0; s0 < nobj; s0 += chunk) {
                const size_t m = std::min<size_t>(chunk, nobj - s0);
                items.resize(m);
                for (size_t j = 0; j < m; j++) items[j] = acl_item_t{(uint16_t)rtype, (uint16_t)perm, rids[i], (uint16_t)stype, srl, (uint32_t)(s0 + j)};
                rc = check_candidates(h, c, comm, items, &ans, &err, &cst);
                if (rc) return rc;
                add_stats(&st, cst);
                for (size_t j = 0; j < m; j++) {
                    if (s0 + j == wid) continue;
                    if (err[j] && strict) return subjects_error(err[j], rids[i], (uint32_t)(s0 + j));
                    if (err[j] || ans[j] != ACL_PERM_HAS_PERMISSION) ex[i * bitmap_words + ((s0 + j) >> 5)] |= 1u << ((s0 + j) & 31u);
                }
            }
        }
        HIP_TRY(hipMemcpy(d_excluded_out, ex.data(), ex.size() * 4, hipMemcpyHostToDevice));
    }
    if (flags_out)
        for (size_t i = 0; i < n; i++) flags_out[i] = wild[i] ? (uint8_t)ACL_SUBJECTS_WILDCARD : (uint8_t)0;
    c->stats.lookup_requests += n;
    c->stats.levels_last = st.levels;
    if (stats_out) *stats_out = st;
    return ACL_OK;
}

int acl_shard_subjects_bulk_rccl(acl_engine_t *h, int rtype, int perm, int stype, int srel, const uint32_t *rids, size_t n, void *d_bitmaps_out, size_t bitmap_words,
                                 uint8_t *flags_out, void *d_excluded_out, acl_shard_bulk_stats_t *stats_out) {
    if (h->store_only) return fail(ACL_ERR_UNAVAILABLE, "engine was opened store-only (no GPU): LookupSubjects is unavailable");
    acl_shard_comm_t comm{};
    int rc = shard_rccl_comm(h, "acl_shard_subjects_bulk_rccl", &comm);
    if (rc) return rc;
    return acl_shard_subjects_bulk(h, &comm, rtype, perm, stype, srel, rids, n, d_bitmaps_out, bitmap_words, flags_out, d_excluded_out, stats_out);
}

}  // extern "C"

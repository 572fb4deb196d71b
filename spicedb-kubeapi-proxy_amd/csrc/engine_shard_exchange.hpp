// engine_shard_exchange.hpp -- what the native sharded loops share (engine_shard_native.cpp: Check and LookupResources; engine_shard_subjects.cpp:
// LookupSubjects): one batch's exchange machinery with the attempt / burst / settle / grow cycle that drives it (Exchange::walk), the statistics fold, and
// the Check loop the lookups confirm their candidates with.
#pragma once
#include "engine_internal.hpp"

namespace aclint {

constexpr uint32_t kCtrlWords = 4;  // per level: total exported, any produced, overflow code, largest block

// The iterations of one walk: first, first + step, ... up to `last`; bursts are counted in exchanges (a level of Check and LookupSubjects, a VISIT / EXPAND
// pair of LookupResources): `burst` of them before the first host synchronisation, `burst_next` before every further one
struct WalkShape {
    uint32_t first, step, last, burst, burst_next;
};

// One batch's exchange machinery: buffers, the per-level "are entries expected?" plan, the collectives.
//   headers  ALWAYS travel (16 bytes per peer): they carry the counts, the produced flag and the overflow code, so termination and
//            retry decisions are taken on the device, identically on every shard;
//   entries  travel only on levels the PLAN expects to export something.  The plan is the previous batch's record (the proxy's request
//            streams repeat their shape: pods -> namespaces / groups cross shards on the first levels, nested groups stay on theirs): a
//            fixed-capacity collective over world x cap entries per level was the price of deciding on the device, and most levels paid
//            it for nothing.  A level that exports after all raises code 4 in every shard's control record and the batch is redone with
//            entries on every level.
struct Exchange {
    acl_engine *h;
    PassCtx *c;
    const acl_shard_comm_t *comm;
    uint32_t world, rank, cap = 0;
    bool a2a = false;     // per-destination blocks through comm->all_to_all (Check only); else one block per shard through all_gather
    acl_shard_bulk_stats_t *st;
    std::vector<uint8_t> *plan;  // [level] 1 = exchange entries; empty = always

    uint32_t nblk() const { return a2a ? world : 1u; }
    // c->xcap is what a shard may export per level IN ALL: the all-gather form moves it whole to every shard, the all-to-all form cuts it into
    // one block per destination -- `world` times fewer bytes on the wire for the same capacity
    void size_blocks() { cap = a2a ? std::max<uint32_t>(8, c->xcap / world) : c->xcap; }
    int alloc() {
        HIP_TRY(c->d_xsend.ensure((size_t)nblk() * cap));
        HIP_TRY(c->d_xrecv.ensure((size_t)world * cap));
        HIP_TRY(c->d_xhsend.ensure(std::max<uint32_t>(world, 64)));
        HIP_TRY(c->d_xhrecv.ensure(std::max<uint32_t>(world, 64)));
        HIP_TRY(c->d_xctrl.ensure((size_t)kLevelSlots * kCtrlWords));
        if (!c->h_xctrl.p) HIP_TRY(c->h_xctrl.ensure((size_t)kLevelSlots * kCtrlWords * sizeof(uint32_t)));
        return ACL_OK;
    }
    DevShard shard() const {
        DevShard sh = dev_shard(h, c, c->d_xsend.p, cap);
        sh.by_dest = a2a ? 1u : 0u;
        return sh;
    }
    bool wants_data(uint32_t it) const { return plan->empty() || it >= plan->size() || (*plan)[it]; }
    // after iteration `it` wrote its exports: headers, (entries), import + control record.  `import`: (hdrs, data, have_data, ctrl)
    template <typename Import>
    int run(uint32_t it, Import import) {
        const uint32_t *status = c->d_status.p;
        launch_xhdr(c->stream, c->d_xhsend.p, nblk(), status + 2 * kLevelSlots + 1, status + kLevelSlots + it, status + 2 * kLevelSlots);
        int rc = a2a ? comm->all_to_all(comm->user, c->d_xhsend.p, c->d_xhrecv.p, sizeof(uint4), (void *)c->stream)
                     : comm->all_gather(comm->user, c->d_xhsend.p, c->d_xhrecv.p, sizeof(uint4), (void *)c->stream);
        if (rc) return rc;
        const bool data = wants_data(it);
        if (data) {
            rc = a2a ? comm->all_to_all(comm->user, c->d_xsend.p, c->d_xrecv.p, (size_t)cap * sizeof(uint4), (void *)c->stream)
                     : comm->all_gather(comm->user, c->d_xsend.p, c->d_xrecv.p, (size_t)cap * sizeof(uint4), (void *)c->stream);
            if (rc) return rc;
            st->exchanged_bytes += (uint64_t)world * cap * sizeof(uint4);
            st->data_exchanges++;
        }
        st->exchanged_bytes += (uint64_t)world * sizeof(uint4);
        st->exchanges++;
        import(c->d_xhrecv.p, c->d_xrecv.p, data, c->d_xctrl.p + (size_t)it * kCtrlWords);
        return ACL_OK;
    }
    // reads the control records of iterations first, first + step, ... last after a burst; returns 0 = go on, 1 = done at *done_at, 2 = redo
    int settle(uint32_t first, uint32_t last, uint32_t step, uint32_t *done_at, uint32_t *redo_code, uint32_t *redo_max, std::vector<uint8_t> *seen) {
        const uint32_t *hc = (const uint32_t *)c->h_xctrl.p;
        for (uint32_t it = first; it <= last; it += step) {
            const uint32_t *k = hc + (size_t)it * kCtrlWords;
            st->entries_exchanged += k[0];
            if (seen->size() <= it) seen->resize(it + 1, 0);
            (*seen)[it] = k[0] ? 1 : 0;
            if (k[2]) {  // some shard overflowed (frontier, export block, a row beyond the enumeration limit, the combine pools) or exported on a level planned without entries
                *redo_code = (k[2] & 2u) ? 2u : (k[2] & kOverflowPools) ? kOverflowPools : (k[2] & 1u) ? 1u : (k[2] & kOverflowExport) ? kOverflowExport : 4u;
                *redo_max = std::max(*redo_max, k[3]);
                return 2;
            }
            if (k[0] == 0 && k[1] == 0) {
                *done_at = it;
                return 1;
            }
        }
        return 0;
    }
    // every shard saw the same control records, so every shard grows the same things and redoes the batch
    int grow(uint32_t redo_code, uint32_t redo_max, int attempt) {
        if (redo_code == 2) return fail(ACL_ERR_RESOURCE_EXHAUSTED, "a relationship row exceeds the per-task enumeration limit");
        st->retries++;
        if (attempt > 8) return fail(ACL_ERR_RESOURCE_EXHAUSTED, "sharded frontier / export capacity exceeded after 8 retries");
        c->stats.overflow_retries++;
        if (redo_code == 4) {
            plan->clear();  // exports where none were expected: entries on every level from now on
            return ACL_OK;
        }
        if (redo_code == kOverflowPools) {  // a shard ran out of combine nodes / leaf cells: four times the pools (every shard alike)
            c->shard_pool_shift += 2;
            return ACL_OK;
        }
        if (redo_max > cap) {  // (kOverflowExport, or a frontier that ran out on the same level: the block first)
            uint32_t nc = cap;
            while (nc < redo_max + redo_max / 4 && nc < (1u << 27)) nc <<= 1;
            c->xcap = a2a ? (uint32_t)std::min<uint64_t>((uint64_t)nc * world, 1u << 30) : nc;  // (xcap = entries a shard may export per level in all)
            return ACL_OK;
        }
        return alloc_frontier(h, c, c->frontier_entries * 4);
    }
    // The cycle the three native walks share, in the style of level_loop (engine_internal.hpp): size and allocate the blocks, zero the control records,
    // begin(); then bursts of iterations -- per iteration the export counters are zeroed and level(it) enqueues the walk's launches around its run(it, import)
    // -- with ONE host synchronisation per burst, until settle() finds the iteration that neither produced nor exported (or w.last is reached).  A burst that
    // asks for a redo is put to redo(code, max, attempt): 0 = grow() and walk again from begin(), anything else ends the walk with that value.  The next
    // call's plan is what this walk exported where; *done_at is the iteration it ended at.
    template <typename Begin, typename Level, typename Redo>
    int walk(const WalkShape &w, Begin begin, Level level, Redo redo, uint32_t *done_at) {
        std::vector<uint8_t> seen;
        for (int attempt = 0;; attempt++) {
            size_blocks();
            int rc = alloc();
            if (rc) return rc;
            HIP_TRY(hipMemsetAsync(c->d_xctrl.p, 0, (size_t)kLevelSlots * kCtrlWords * sizeof(uint32_t), c->stream));
            rc = begin();
            if (rc) return rc;
            uint32_t next = w.first, burst = w.burst, redo_max = 0, redo_code = 0;
            int verdict = 0;
            seen.clear();
            while (!verdict) {
                const uint32_t last = std::min<uint32_t>(w.last, next + w.step * (burst - 1));
                for (uint32_t it = next; it <= last; it += w.step) {
                    HIP_TRY(hipMemsetAsync(c->d_status.p + 2 * kLevelSlots + 1, 0, (1 + kMaxShards) * sizeof(uint32_t), c->stream));
                    rc = level(it);
                    if (rc) return rc;
                }
                HIP_TRY(hipMemcpyAsync(c->h_xctrl.p, c->d_xctrl.p, (size_t)kLevelSlots * kCtrlWords * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(hipStreamSynchronize(c->stream));
                ev_collect(c);
                st->host_syncs++;
                verdict = settle(next, last, w.step, done_at, &redo_code, &redo_max, &seen);
                if (!verdict && last == w.last) {
                    *done_at = w.last;
                    verdict = 1;
                }
                next = last + w.step;
                burst = w.burst_next;
            }
            if (verdict == 1) break;
            rc = redo(redo_code, redo_max, attempt);
            if (rc) return rc;
            rc = grow(redo_code, redo_max, attempt);
            if (rc) return rc;
        }
        *plan = seen;  // the next batch exchanges entries where this one exported some (iterations beyond: always)
        return ACL_OK;
    }
};

// (The sharded level loops merge duplicates like check_pass does -- dedup_table, engine_internal.hpp.  Merging is local to a shard: the entries struck
//  have the subtree of the one that stays, so the shards need not agree on it.)
inline uint32_t first_xcap(PassCtx *c) {
    if (!c->xcap) {
        const char *e = getenv("ACL_SHARD_XCAP");  // test knob: a tiny first export block forces the grow-and-redo path
        c->xcap = e && atoi(e) > 0 ? (uint32_t)std::max(8, atoi(e)) : 1u << 16;
    }
    return c->xcap;
}

// the counters of a call that sum over its passes, chunks and confirming Checks (levels and export_capacity: each caller has its own rule)
inline void add_stats(acl_shard_bulk_stats_t *dst, const acl_shard_bulk_stats_t &src) {
    dst->exchanges += src.exchanges;
    dst->data_exchanges += src.data_exchanges;
    dst->entries_exchanged += src.entries_exchanged;
    dst->exchanged_bytes += src.exchanged_bytes;
    dst->host_syncs += src.host_syncs;
    dst->retries += src.retries;
}

// the native Check loop on context c (the caller holds the shard call's locks; engine_shard_native.cpp)
int shard_check_core(acl_engine_t *h, PassCtx *c, const acl_shard_comm_t *comm, const void *d_items, size_t n, void *d_perm_out, void *d_err_out,
                     acl_shard_bulk_stats_t *stats_out);
// one sharded Check over `items` (the same on every shard), as the lookups confirm the candidates of a permission with `&` / `-` / `.all()`: answers and
// per-item errors by index, the Check's own statistics in *check_stats
int check_candidates(acl_engine_t *h, PassCtx *c, const acl_shard_comm_t *comm, const std::vector<acl_item_t> &items, std::vector<uint8_t> *perm, std::vector<int32_t> *err,
                     acl_shard_bulk_stats_t *check_stats);
// the built-in RCCL communicator of an engine after acl_shard_rccl_init (else ACL_ERR_FAILED_PRECONDITION, naming `who`)
int shard_rccl_comm(acl_engine_t *h, const char *who, acl_shard_comm_t *out);

}  // namespace aclint

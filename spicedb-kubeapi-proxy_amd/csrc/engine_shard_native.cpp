// engine_shard_native.cpp -- the sharded level loop INSIDE libaclgpu.so (north star: "the graph shards by
// object-type hash across GPUs with RCCL allgather of cross-shard frontiers over xGMI").
//
// Round 1 drove the protocol from the host (aclgpu/sharded.py): per level two host-synchronising collectives (counts, then
// data) plus a stream sync -- on 8 logical shards 9.5 ms per 256 k batch against 0.6 ms for a replica.  Here:
//   * ONE fixed-capacity all-gather per level: every shard contributes [header | cap entries]; the header (entries exported,
//     produced flag, overflow code) is written by a kernel, so the counts ride with the data;
//   * imports and the level's control record {total exported, any produced, overflow, largest export} are computed on the
//     device from the gathered headers -- identical on every shard, so all shards take the same decisions without talking;
//   * the host enqueues a whole burst of levels (sized by the previous batch's depth) and synchronises ONCE per burst:
//     levels past the end find empty frontiers and cost a few microseconds each;
//   * has / err are MAX-reduced across shards once per batch (HAS beats error beats NO is a max).
// The collective is a pair of callbacks (acl_shard_comm_t): RCCL over xGMI in production (acl_shard_rccl_*, below: librccl
// is dlopen'ed, the library has no link-time dependency on it), an in-process copy between logical shards in the
// single-GPU tests -- the loop, kernels and decisions are the same code either way.
#include <dlfcn.h>
#include <rccl/rccl.h>

#include "engine_shard_exchange.hpp"

namespace {

struct Rccl {
    void *lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    // (optional: the all-to-all form of the exchange)
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    std::string err;
};

Rccl *rccl() {
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        // the copy already in the process (PyTorch-ROCm bundles one) wins: two RCCLs in one process would each open the GPUs
        for (const char *name : {"librccl.so", "librccl.so.1"}) {
            r.lib = dlopen(name, RTLD_NOW | RTLD_NOLOAD);
            if (r.lib) break;
        }
        if (!r.lib)
            for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
                r.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
                if (r.lib) break;
            }
        if (!r.lib) {
            r.err = std::string("librccl.so not found: ") + (dlerror() ? dlerror() : "");
            return;
        }
        auto sym = [&](const char *n) {
            void *p = dlsym(r.lib, n);
            if (!p) r.err = std::string("librccl.so lacks ") + n;
            return p;
        };
        r.GetUniqueId = (decltype(r.GetUniqueId))sym("ncclGetUniqueId");
        r.CommInitRank = (decltype(r.CommInitRank))sym("ncclCommInitRank");
        r.CommDestroy = (decltype(r.CommDestroy))sym("ncclCommDestroy");
        r.AllGather = (decltype(r.AllGather))sym("ncclAllGather");
        r.AllReduce = (decltype(r.AllReduce))sym("ncclAllReduce");
        r.GetErrorString = (decltype(r.GetErrorString))sym("ncclGetErrorString");
        r.Send = (decltype(r.Send))dlsym(r.lib, "ncclSend");
        r.Recv = (decltype(r.Recv))dlsym(r.lib, "ncclRecv");
        r.GroupStart = (decltype(r.GroupStart))dlsym(r.lib, "ncclGroupStart");
        r.GroupEnd = (decltype(r.GroupEnd))dlsym(r.lib, "ncclGroupEnd");
        r.CommCount = (decltype(r.CommCount))dlsym(r.lib, "ncclCommCount");
    });
    return &r;
}

int rccl_all_gather(void *user, const void *send, void *recv, size_t bytes, void *stream) {
    Rccl *r = rccl();
    ncclResult_t e = r->AllGather(send, recv, bytes, ncclUint8, (ncclComm_t)user, (hipStream_t)stream);
    return e == ncclSuccess ? ACL_OK : fail(ACL_ERR_INTERNAL, std::string("ncclAllGather: ") + r->GetErrorString(e));
}
int rccl_all_reduce_max(void *user, void *buf, size_t n, void *stream) {
    Rccl *r = rccl();
    ncclResult_t e = r->AllReduce(buf, buf, n, ncclUint8, ncclMax, (ncclComm_t)user, (hipStream_t)stream);
    return e == ncclSuccess ? ACL_OK : fail(ACL_ERR_INTERNAL, std::string("ncclAllReduce: ") + r->GetErrorString(e));
}
// block r of `send` goes to rank r, block r of `recv` comes from rank r: one grouped ncclSend / ncclRecv pair per peer (xGMI is point to point:
// this IS the native shape of an all-to-all there)
int rccl_all_to_all(void *user, const void *send, void *recv, size_t bytes, void *stream) {
    Rccl *r = rccl();
    if (!r->Send || !r->Recv || !r->GroupStart || !r->GroupEnd || !r->CommCount) return fail(ACL_ERR_UNAVAILABLE, "librccl.so lacks ncclSend / ncclRecv / ncclGroupStart");
    int world = 0;
    ncclResult_t e = r->CommCount((ncclComm_t)user, &world);
    if (e == ncclSuccess) e = r->GroupStart();
    for (int p = 0; p < world && e == ncclSuccess; p++) {
        e = r->Send((const char *)send + (size_t)p * bytes, bytes, ncclUint8, p, (ncclComm_t)user, (hipStream_t)stream);
        if (e == ncclSuccess) e = r->Recv((char *)recv + (size_t)p * bytes, bytes, ncclUint8, p, (ncclComm_t)user, (hipStream_t)stream);
    }
    if (e == ncclSuccess) e = r->GroupEnd();
    return e == ncclSuccess ? ACL_OK : fail(ACL_ERR_INTERNAL, std::string("all-to-all (ncclSend / ncclRecv): ") + r->GetErrorString(e));
}

}  // namespace

namespace {

// One pass of the native Check loop over n items.  `merging`: duplicate (request, state, level) entries of a level are struck behind its imports
// (n <= kDedupBatch then: the merge key holds 14 request bits).  Without it, a frontier or pool overflow answers kRetryMerging -- at once for a batch of
// one merge slice, behind one growth of the frontier or the pools for a larger one; taken from the control records, so on every shard alike.  An outgrown
// export block is no such overflow: it is grown and the pass redone, merging or not.
int shard_check_pass(acl_engine_t *h, PassCtx *c, const acl_shard_comm_t *comm, const void *d_items, size_t n, void *d_perm_out, void *d_err_out,
                     acl_shard_bulk_stats_t *stats_out, bool merging) {
    int rc = ACL_OK;
    acl_shard_bulk_stats_t st{};
    Exchange X{h, c, comm, h->shard.world, h->shard.rank, 0, comm->all_to_all != nullptr && h->shard.world <= kMaxShards && h->shard_a2a, &st, &c->xplan_fwd};
    // Schemas with `&` / `-` / `.all()` on the sharded graph (round 5).  A state with a combine program is visited on the shard
    // that owns its type: that shard appends the CombineNode and hands out the state's leaf cells from ITS range of one global cell space --
    // cell ids [n + r cell_cap, n + (r + 1) cell_cap) belong to shard r, and a cell id is what a frontier entry carries where the request
    // was, so the leaves' sub-walks cross shards like any other entry.  Every shard keeps has / err bytes for the WHOLE cell space and sets
    // whatever a sub-walk answers locally; behind the walk a byte-wise max makes the arrays identical everywhere (HAS / error bytes are only ever
    // raised during the walk), the node lists are all-gathered, and every shard resolves ALL nodes deepest iteration first -- redundantly and
    // identically, so nothing travels between the resolve iterations.
    const bool combine = h->snap.has_combine;
    const uint32_t world = h->shard.world;
    size_t node_cap = 0, cell_cap = 0, cells = 0;
    HIP_TRY(c->d_has.ensure(std::max<size_t>(n, 4096)));
    HIP_TRY(c->d_err.ensure(std::max<size_t>(n, 4096)));
    if ((uint64_t)n > c->frontier_entries) {
        rc = alloc_frontier(h, c, (uint64_t)n * 4);
        if (rc) return rc;
    }
    first_xcap(c);
    bool grown = false;  // this pass grew the frontier or the pools already
    DevGraph g;
    DevFrontier f;
    DevShard sh;
    uint32_t dedup_bits = 0, done_at = 0;
    auto begin = [&]() -> int {
        g = h->dev_graph(c);
        if (combine) {
            // (the cell space is memset and max-reduced whole, per batch and shard -- world x 4 x node_cap bytes twice -- whatever the batch creates.  It starts a
            //  quarter of round 5's size; a shard that runs out raises kOverflowPools and the batch is redone with pools x 4 (shard_pool_shift += 2); a batch that used
            //  less than an eighth of its pools gives half of the growth back, below)
            node_cap = std::max<size_t>((size_t)1 << 14, n) << c->shard_pool_shift;
            cell_cap = node_cap * 4;
            cells = (size_t)world * cell_cap;
            if ((uint64_t)n + cells >= 0xFFFFFFF0ull) return fail(ACL_ERR_RESOURCE_EXHAUSTED, "combine cells beyond 2^32 on the sharded graph: smaller batches");
            HIP_TRY(c->d_nodes.ensure(node_cap));
            HIP_TRY(c->d_has.ensure(n + cells));
            HIP_TRY(c->d_err.ensure(n + cells));
            HIP_TRY(c->d_ccount.ensure(2));
            HIP_TRY(hipMemsetAsync(c->d_ccount.p, 0, 2 * sizeof(uint32_t), c->stream));
            HIP_TRY(hipMemsetAsync(c->d_has.p + n, 0, cells, c->stream));  // (the other shards' cells too: the max behind the walk reads every byte)
            HIP_TRY(hipMemsetAsync(c->d_err.p + n, 0, cells, c->stream));
            g.bexpr = c->dev->d_bexpr.p;
            g.nodes = c->d_nodes.p;
            g.node_cap = (uint32_t)node_cap;
            g.cell_cap = (uint32_t)cell_cap;
            g.cell0 = (uint32_t)(n + (size_t)X.rank * cell_cap);
            g.ccount = c->d_ccount.p;
        }
        f = h->dev_frontier(*c);
        sh = X.shard();
        if (merging) {
            int rc = dedup_table(c, combine, &dedup_bits);
            if (rc) return rc;
        }
        ev_begin(c, 0);
        launch_seed(c->stream, g, f, (const uint4 *)d_items, (uint32_t)n, c->d_has.p, c->d_err.p, sh);  // also resets the status block
        ev_end(c);
        return ACL_OK;
    };
    auto level = [&](uint32_t it) -> int {
        ev_begin(c, 1);
        launch_expand(c->stream, g, f, it, c->d_has.p, c->d_err.p, sh);
        ev_end(c);
        int rc = X.run(it, [&](const uint4 *hdrs, const uint4 *data, bool have, uint32_t *ctrl) {
            launch_import_gathered(c->stream, g, f, it, hdrs, data, X.world, X.rank, X.cap, have, ctrl);
        });
        if (rc) return rc;
        if (merging) launch_dedup(c->stream, f, it, c->d_dedup.p, dedup_bits, combine);  // (this level's entries, the imported ones among them)
        c->stats.expand_launches++;
        return ACL_OK;
    };
    auto redo = [&](uint32_t redo_code, uint32_t redo_max, int attempt) -> int {
        // the frontier (or, on a cyclic graph under `&` / `-`, the combine pools) ran out: a batch of one merge slice that outgrew a frontier sized for
        // thousands of entries per item is exploding, a larger one gets one growth first -- then, before growing further, duplicates are merged.
        // An outgrown export block alone (kOverflowExport) is grown by X.grow and the pass redone as it was -- unless the block is what shows the
        // explosion first: where every hop crosses shards a level's exports are its frontier, and a block of 2^16 entries is outgrown ten levels before
        // a frontier of 2^25 is, one redo a level.  So: one level exporting what the default frontier holds per item of a full slice (2^25 / 2^14
        // entries) for every item of a one-slice batch, or a block outgrown for the sixth time (a graph without such cycles outgrows it once per level
        // whose exports exceed all before, a handful), is taken for the same explosion.
        const bool ran_out = redo_code == kOverflowPools || redo_code == 1u;
        const bool block_explodes = redo_code == kOverflowExport && ((n <= kDedupBatch && redo_max >= 2048ull * std::max<size_t>(n, 1)) || attempt >= 5);
        if (!merging && (block_explodes || (ran_out && (n <= kDedupBatch || grown)))) {
            if (stats_out) *stats_out = st;
            return kRetryMerging;
        }
        grown |= ran_out && (redo_code == kOverflowPools || redo_max <= X.cap);  // (X.grow: an outgrown block comes before the frontier)
        return 0;
    };
    rc = X.walk(WalkShape{1, 1, kMaxLevels, std::max<uint32_t>(c->levels_hint, 2), 4}, begin, level, redo, &done_at);
    if (rc) return rc;
    c->levels_hint = done_at;
    st.levels = done_at;
    // HAS beats error beats NO: a byte-wise max across shards, then the answers on every shard
    if (n) {
        rc = comm->all_reduce_max_u8(comm->user, c->d_has.p, n + cells, (void *)c->stream);
        if (rc) return rc;
        rc = comm->all_reduce_max_u8(comm->user, c->d_err.p, n + cells, (void *)c->stream);
        if (rc) return rc;
    }
    if (combine && n) {
        // the shards' node lists: counts first (16-byte headers), then blocks of the largest count; resolved on every shard alike
        HIP_TRY(c->d_xhsend.ensure(std::max<uint32_t>(world, 64)));
        HIP_TRY(c->d_xhrecv.ensure(std::max<uint32_t>(world, 64)));
        launch_node_hdr(c->stream, c->d_xhsend.p, c->d_ccount.p);
        rc = comm->all_gather(comm->user, c->d_xhsend.p, c->d_xhrecv.p, sizeof(uint4), (void *)c->stream);
        if (rc) return rc;
        std::vector<uint4> hh(world);
        HIP_TRY(hipMemcpyAsync(hh.data(), c->d_xhrecv.p, (size_t)world * sizeof(uint4), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        st.host_syncs++;
        uint32_t maxc = 0, max_cells = 0;
        for (const uint4 &x : hh) {
            maxc = std::max(maxc, std::min<uint32_t>(x.x, (uint32_t)node_cap));
            max_cells = std::max(max_cells, x.y);
        }
        if (c->shard_pool_shift && (uint64_t)maxc * 8 < node_cap && (uint64_t)max_cells * 8 < cell_cap) c->shard_pool_shift--;  // (identical on every shard: the headers are)
        if (maxc) {
            HIP_TRY(c->d_nodes_all.ensure((size_t)world * maxc));
            rc = comm->all_gather(comm->user, c->d_nodes.p, c->d_nodes_all.p, (size_t)maxc * sizeof(uint4), (void *)c->stream);
            if (rc) return rc;
            st.exchanged_bytes += (uint64_t)world * maxc * sizeof(uint4);
            DevGraph g = h->dev_graph(c);
            g.bexpr = c->dev->d_bexpr.p;
            for (uint32_t it = std::max<uint32_t>(st.levels, 1); it >= 1; it--) launch_resolve_gathered(c->stream, g, c->d_nodes_all.p, maxc, c->d_xhrecv.p, world, it, c->d_has.p, c->d_err.p);
        }
    }
    ev_begin(c, 0);
    launch_finalize(c->stream, (uint32_t)n, c->d_has.p, c->d_err.p, (uint8_t *)d_perm_out, (int32_t *)d_err_out);
    ev_end(c);
    HIP_TRY(hipStreamSynchronize(c->stream));
    ev_collect(c);
    st.host_syncs++;
    st.export_capacity = X.cap;
    c->stats.check_items += n;
    c->stats.check_passes++;
    c->stats.levels_last = st.levels;
    if (stats_out) *stats_out = st;
    return ACL_OK;
}

}  // namespace

// the native Check loop on context c (the caller holds the shard call's locks): acl_shard_check_bulk, and the forward half of LookupResources over
// a non-monotone permission (candidates + one Check)
int aclint::shard_check_core(acl_engine_t *h, PassCtx *c, const acl_shard_comm_t *comm, const void *d_items, size_t n, void *d_perm_out, void *d_err_out,
                             acl_shard_bulk_stats_t *stats_out) {
    acl_shard_bulk_stats_t st{};
    int rc = shard_check_pass(h, c, comm, d_items, n, d_perm_out, d_err_out, &st, false);
    if (rc != kRetryMerging) {
        if (!rc && stats_out) *stats_out = st;
        return rc;
    }
    // The batch again with duplicates merged behind every level, on slices the merge key can hold (what check_pass does on one device).  Every shard is
    // here: the verdict came from the control records.
    st.retries++;
    c->stats.overflow_retries++;
    for (size_t off = 0; off < n; off += kDedupBatch) {
        const size_t m = std::min<size_t>(kDedupBatch, n - off);
        acl_shard_bulk_stats_t pst{};
        rc = shard_check_pass(h, c, comm, (const uint4 *)d_items + off, m, (uint8_t *)d_perm_out + off, d_err_out ? (int32_t *)d_err_out + off : nullptr, &pst, true);
        if (rc) return rc;
        add_stats(&st, pst);
        st.levels = std::max(st.levels, pst.levels);
        st.export_capacity = std::max(st.export_capacity, pst.export_capacity);
    }
    if (stats_out) *stats_out = st;
    return ACL_OK;
}

int aclint::check_candidates(acl_engine_t *h, PassCtx *c, const acl_shard_comm_t *comm, const std::vector<acl_item_t> &items, std::vector<uint8_t> *perm,
                             std::vector<int32_t> *err, acl_shard_bulk_stats_t *check_stats) {
    perm->assign(items.size(), 0);
    err->assign(items.size(), 0);
    *check_stats = acl_shard_bulk_stats_t{};
    if (items.empty()) return ACL_OK;
    HIP_TRY(c->d_items.ensure(items.size()));
    HIP_TRY(c->d_perm.ensure(items.size()));
    HIP_TRY(c->d_errout.ensure(items.size()));
    HIP_TRY(hipMemcpy(c->d_items.p, items.data(), items.size() * sizeof(acl_item_t), hipMemcpyHostToDevice));
    int rc = shard_check_core(h, c, comm, c->d_items.p, items.size(), c->d_perm.p, c->d_errout.p, check_stats);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(perm->data(), c->d_perm.p, items.size(), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(err->data(), c->d_errout.p, items.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    return ACL_OK;
}

int aclint::shard_rccl_comm(acl_engine_t *h, const char *who, acl_shard_comm_t *out) {
    if (!h->rccl_comm) return fail(ACL_ERR_FAILED_PRECONDITION, std::string(who) + " without acl_shard_rccl_init");
    *out = acl_shard_comm_t{h->rccl_comm, rccl_all_gather, rccl_all_reduce_max, rccl_all_to_all};
    return ACL_OK;
}

extern "C" {

int acl_shard_check_bulk(acl_engine_t *h, const acl_shard_comm_t *comm, const void *d_items, size_t n, void *d_perm_out, void *d_err_out,
                         acl_shard_bulk_stats_t *stats_out) {
    if (!comm || !comm->all_gather || !comm->all_reduce_max_u8) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_shard_check_bulk: communicator callbacks missing");
    if (n && (!d_items || !d_perm_out)) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_shard_check_bulk: NULL buffer");
    if (n > 0xFFFFFFFFu) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_shard_check_bulk: batch too large");
    ShardCall sc;
    int rc = sc.begin(h, true, false, true);
    if (rc) return rc;
    return shard_check_core(h, sc.c, comm, d_items, n, d_perm_out, d_err_out, stats_out);
}

// LookupResources (pkg/authz/lookups.go:49-83) for n subjects of one class on the sharded graph, the whole reverse level loop inside the
// library.  Iteration 1 expands the seeds; then pairs (VISIT: first visits marked, states whose parents' rows also live on other shards
// exported -> exchange -> import of the foreign states this shard holds parent rows for | EXPAND) until a visit step neither produced nor
// exported anything on any shard.  A visited state goes to the shards that hold parent rows for its slot: per-destination blocks through the
// communicator's all_to_all, or -- without one -- one block to everybody, filtered by the importers.
// d_bitmaps_out: n rows of bitmap_words words on the device, the same on every shard afterwards (the rows exist on the resource type's owner
// only; a byte-wise max hands them to everybody).
int acl_shard_lookup_bulk(acl_engine_t *h, const acl_shard_comm_t *comm, int rtype, int perm, int stype, int srel, const uint32_t *sids, size_t n,
                          void *d_bitmaps_out, size_t bitmap_words, acl_shard_bulk_stats_t *stats_out) {
    if (!comm || !comm->all_gather || !comm->all_reduce_max_u8) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_shard_lookup_bulk: communicator callbacks missing");
    if (n && (!sids || !d_bitmaps_out)) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_shard_lookup_bulk: NULL buffer");
    ShardCall scall;
    int rc = scall.begin(h, true, true, true);
    if (rc) return rc;
    PassCtx *c = scall.c;
    const Schema &sc = h->store.schema();
    if (rtype < 0 || rtype >= (int)sc.defs.size() || stype < 0 || stype >= (int)sc.defs.size() || perm < 0 || perm >= (int)sc.defs[rtype].members.size() ||
        srel >= (int)sc.defs[stype].members.size())
        return fail(ACL_ERR_FAILED_PRECONDITION, "lookup: unknown type, permission or subject relation");
    const uint32_t target = (uint32_t)sc.slot(rtype, perm);
    const uint32_t key = sc.subject_key(stype, srel < 0 ? kNoRelation : srel);
    const size_t need = ((size_t)h->store.objects(rtype).count() + 31) / 32;
    if (n && bitmap_words < need) return fail(ACL_ERR_INVALID_ARGUMENT, "lookup: bitmap too small (" + std::to_string(need) + " words needed)");
    const size_t vwords = std::max<size_t>((size_t)((h->snap.visited_bits + 31) / 32), 1);
    if (n * vwords > ((size_t)1 << 30)) return fail(ACL_ERR_RESOURCE_EXHAUSTED, "lookup batch too large for one pass (visited bitmaps > 4 GiB)");
    acl_shard_bulk_stats_t st{};
    // all-to-all by parent-row owner (round 4): a visited state travels to the shards that hold parent rows for its slot (Snapshot::rdest), one
    // block per destination, instead of to everybody; the all-gather form remains for communicators without all_to_all and worlds beyond 64
    Exchange X{h, c, comm, h->shard.world, h->shard.rank, 0, comm->all_to_all != nullptr && h->shard.world <= kMaxShards && h->shard_a2a, &st, &c->xplan_rev};
    if (n > c->frontier_entries) {
        rc = alloc_frontier(h, c, n * 4);
        if (rc) return rc;
    }
    HIP_TRY(c->d_visited.ensure(std::max<size_t>(n, 1) * vwords));
    HIP_TRY(c->d_sids.ensure(std::max<size_t>(n, 1)));
    HIP_TRY(c->h_in.ensure(std::max<size_t>(n, 1) * sizeof(uint32_t)));
    if (n) std::memcpy(c->h_in.p, sids, n * sizeof(uint32_t));
    HIP_TRY(hipMemcpyAsync(c->d_sids.p, c->h_in.p, std::max<size_t>(n, 1) * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    first_xcap(c);
    constexpr uint32_t kMaxIter = 2 * (kMaxLevels + 1);  // (iteration slots: kLevelSlots = 128)
    DevFrontier f;
    DevReverse r;
    DevShard sh;
    uint32_t done_at = 0;
    rc = X.walk(
        WalkShape{2, 2, kMaxIter, std::max<uint32_t>(c->rev_levels_hint, 2), 3},  // VISIT iterations 2, 4, ...: a burst is so many VISIT / EXPAND pairs
        [&]() -> int {
            f = h->dev_frontier(*c);
            r = h->dev_reverse(c, (uint32_t)vwords);
            sh = X.shard();
            HIP_TRY(hipMemsetAsync(c->d_visited.p, 0, std::max<size_t>(n, 1) * vwords * 4, c->stream));
            launch_rev_seed(c->stream, f, c->d_sids.p, (uint32_t)n, key);  // seeds + status block
            ev_begin(c, 1);
            launch_rev_expand(c->stream, r, f, 1, REV_EXPAND, sh);  // iteration 1: the seeds
            ev_end(c);
            c->stats.expand_launches++;
            return ACL_OK;
        },
        [&](uint32_t it) -> int {
            ev_begin(c, 1);
            launch_rev_expand(c->stream, r, f, it, REV_VISIT, sh);
            ev_end(c);
            int rc = X.run(it, [&](const uint4 *hdrs, const uint4 *data, bool have, uint32_t *ctrl) {
                launch_rev_import_gathered(c->stream, r, f, it, hdrs, data, X.world, X.rank, X.cap, have, ctrl);
            });
            if (rc) return rc;
            ev_begin(c, 1);
            launch_rev_expand(c->stream, r, f, it + 1, REV_EXPAND, sh);
            ev_end(c);
            c->stats.expand_launches += 2;
            return ACL_OK;
        },
        [](uint32_t, uint32_t, int) { return 0; }, &done_at);
    if (rc) return rc;
    c->rev_levels_hint = std::max<uint32_t>(1, done_at / 2);
    st.levels = done_at / 2;
    // result rows: the resource type's owner holds them; everybody else contributes zeros to a byte-wise max
    if (n) {
        const size_t woff = h->snap.slot_bit_base[target] / 32;
        const size_t cw = std::min(need, ((size_t)h->snap.slot_nobjects[target] + 31) / 32);  // only the ids the snapshot's slot covers can be marked
        HIP_TRY(hipMemsetAsync(d_bitmaps_out, 0, n * bitmap_words * 4, c->stream));
        if (cw && shard_of_type(sc.defs[rtype].name, h->shard.world) == h->shard.rank)
            HIP_TRY(hipMemcpy2DAsync(d_bitmaps_out, bitmap_words * 4, c->d_visited.p + woff, vwords * 4, cw * 4, n, hipMemcpyDeviceToDevice, c->stream));
        rc = comm->all_reduce_max_u8(comm->user, d_bitmaps_out, n * bitmap_words * 4, (void *)c->stream);
        if (rc) return rc;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    ev_collect(c);
    st.host_syncs++;
    uint64_t export_cap = X.cap;  // (entries per exchange block, as the Check and LookupSubjects loops report it: all three size their blocks from c->xcap)
    // Schemas with `&` / `-` (round 5): the reverse walk follows only POSITIVE occurrences (plan_reverse.cpp), so the rows are candidates -- a
    // superset.  The answer is the candidates the forward walk grants: every shard holds the same rows by now, builds the same items and takes
    // part in ONE sharded Check (shard_check_core: the collectives stay in lockstep); bits of everything but HAS are cleared (as lookup_refine on
    // the unsharded graph).
    if (n && h->snap.has_combine && !h->snap.slot_nonmono.empty() && h->snap.slot_nonmono[target]) {
        std::vector<uint32_t> rows(n * bitmap_words);
        HIP_TRY(hipMemcpy(rows.data(), d_bitmaps_out, rows.size() * 4, hipMemcpyDeviceToHost));
        const uint16_t sr = (uint16_t)(srel < 0 ? ACL_NO_RELATION : srel);
        std::vector<acl_item_t> items;
        for (size_t i = 0; i < n; i++)
            for (size_t w = 0; w < bitmap_words; w++)
                for (uint32_t m = rows[i * bitmap_words + w]; m; m &= m - 1)
                    items.push_back(acl_item_t{(uint16_t)rtype, (uint16_t)perm, (uint32_t)(w * 32 + (size_t)__builtin_ctz(m)), (uint16_t)stype, sr, sids[i]});
        if (items.size() > 0xFFFFFFF0ull) return fail(ACL_ERR_RESOURCE_EXHAUSTED, "lookup over a non-monotone permission: too many candidates for one Check");
        if (!items.empty()) {
            std::vector<uint8_t> ans;
            std::vector<int32_t> errs;
            acl_shard_bulk_stats_t cst{};
            rc = check_candidates(h, c, comm, items, &ans, &errs, &cst);
            if (rc) return rc;
            if (!h->lenient_lookup)  // (a candidate whose Check errs fails the call, as on the unsharded graph: lookup_refine; every shard holds the same answers: all of them fail, or none)
                for (size_t k = 0; k < errs.size(); k++)
                    if (errs[k]) return lookup_candidate_error(h, errs[k], items[k].resource_id, items[k].subject_id);
            add_stats(&st, cst);
            export_cap = std::max<uint64_t>(export_cap, cst.export_capacity);
            size_t k = 0;
            for (size_t i = 0; i < n; i++)
                for (size_t w = 0; w < bitmap_words; w++) {
                    uint32_t &word = rows[i * bitmap_words + w];
                    for (uint32_t m = word; m; m &= m - 1, k++)
                        if (ans[k] != ACL_PERM_HAS_PERMISSION) word &= ~(m & (0u - m));
                }
            HIP_TRY(hipMemcpy(d_bitmaps_out, rows.data(), rows.size() * 4, hipMemcpyHostToDevice));
        }
    }
    st.export_capacity = export_cap;
    c->stats.lookup_requests += n;
    c->stats.levels_last = st.levels;
    if (stats_out) *stats_out = st;
    return ACL_OK;
}

// ---- the built-in communicator: RCCL (one rank per GPU, xGMI between them)
int acl_shard_rccl_unique_id(void *id_out) {
    if (!id_out) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_shard_rccl_unique_id: NULL");
    Rccl *r = rccl();
    if (!r->lib || !r->err.empty()) return fail(ACL_ERR_UNAVAILABLE, r->err.empty() ? "RCCL unavailable" : r->err);
    ncclUniqueId id;
    ncclResult_t e = r->GetUniqueId(&id);
    if (e != ncclSuccess) return fail(ACL_ERR_INTERNAL, std::string("ncclGetUniqueId: ") + r->GetErrorString(e));
    static_assert(sizeof(ncclUniqueId) == ACL_RCCL_UNIQUE_ID_BYTES, "ncclUniqueId size");
    std::memcpy(id_out, &id, sizeof id);
    return ACL_OK;
}

int acl_shard_rccl_init(acl_engine_t *h, const void *unique_id, uint32_t rank, uint32_t world) {
    if (!unique_id) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_shard_rccl_init: NULL id");
    if (h->store_only) return fail(ACL_ERR_UNAVAILABLE, "engine was opened store-only (no GPU)");
    Rccl *r = rccl();
    if (!r->lib || !r->err.empty()) return fail(ACL_ERR_UNAVAILABLE, r->err.empty() ? "RCCL unavailable" : r->err);
    int rc = acl_shard_configure(h, rank, world);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->dev0().device));
    std::lock_guard<std::mutex> lk(h->shard_mu);
    if (h->rccl_comm) {
        (void)r->CommDestroy((ncclComm_t)h->rccl_comm);
        h->rccl_comm = nullptr;
    }
    ncclUniqueId id;
    std::memcpy(&id, unique_id, sizeof id);
    ncclComm_t comm = nullptr;
    ncclResult_t e = r->CommInitRank(&comm, (int)world, id, (int)rank);
    if (e != ncclSuccess) return fail(ACL_ERR_INTERNAL, std::string("ncclCommInitRank: ") + r->GetErrorString(e));
    h->rccl_comm = comm;
    return ACL_OK;
}

int acl_shard_rccl_destroy(acl_engine_t *h) {
    std::lock_guard<std::mutex> lk(h->shard_mu);
    if (h->rccl_comm) {
        (void)rccl()->CommDestroy((ncclComm_t)h->rccl_comm);
        h->rccl_comm = nullptr;
    }
    return ACL_OK;
}

int acl_shard_check_bulk_rccl(acl_engine_t *h, const void *d_items, size_t n, void *d_perm_out, void *d_err_out, acl_shard_bulk_stats_t *stats_out) {
    acl_shard_comm_t comm{};
    int rc = shard_rccl_comm(h, "acl_shard_check_bulk_rccl", &comm);
    if (rc) return rc;
    return acl_shard_check_bulk(h, &comm, d_items, n, d_perm_out, d_err_out, stats_out);
}

int acl_shard_lookup_bulk_rccl(acl_engine_t *h, int rtype, int perm, int stype, int srel, const uint32_t *sids, size_t n, void *d_bitmaps_out, size_t bitmap_words,
                               acl_shard_bulk_stats_t *stats_out) {
    acl_shard_comm_t comm{};
    int rc = shard_rccl_comm(h, "acl_shard_lookup_bulk_rccl", &comm);
    if (rc) return rc;
    return acl_shard_lookup_bulk(h, &comm, rtype, perm, stype, srel, sids, n, d_bitmaps_out, bitmap_words, stats_out);
}

}  // extern "C"

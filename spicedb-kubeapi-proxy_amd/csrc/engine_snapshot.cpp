// engine_snapshot.cpp -- the device snapshot: upload and patching, background compaction, the reverse rows, and the start
// and end of an evaluating call (Eval: state_mu shared + a context from the pool).
#include "engine_internal.hpp"

namespace aclint {

bool snapshot_current(acl_engine *h, bool need_reverse) {
    if (!h->snap_valid || !h->all_dev_valid() || h->snap.revision != h->store.revision()) return false;
    const int64_t now = h->store.now();
    if (now < h->snap.valid_lo || now >= h->snap.valid_hi) return false;
    return !need_reverse || h->all_rev_uploaded();
}

// Uploads the regions a patch touched.  A region is one hipMemcpyAsync (a few microseconds of API time each): past a few
// hundred regions of one array the whole array goes instead (70 MB of snapshot cross PCIe in ~2 ms; 6 000 regions took 28 ms).
// *fits = false when a host array outgrew its device allocation (the caller uploads everything).
struct SnapArrays {
    DevArray<uint32_t> *meta, *edges, *buckets, *rmeta, *redges;
    DevArray<FwdOp> *ops;
};
static hipError_t upload_patches(const Snapshot &sn, const std::vector<Patch> &patches, const SnapArrays &a, bool with_reverse, hipStream_t s, bool *fits) {
    size_t cnt[6] = {0, 0, 0, 0, 0, 0};
    for (const Patch &p : patches) cnt[p.array]++;
    constexpr size_t kWhole = 256;
    hipError_t err = hipSuccess;
    auto whole = [&](auto *dev, const auto &host) {
        if (!dev->p || host.size() > dev->n) *fits = false;
        else if (hipError_t e = hipMemcpyAsync(dev->p, host.data(), host.size() * sizeof(host[0]), hipMemcpyHostToDevice, s); e != hipSuccess) err = e;
    };
    if (cnt[Patch::META] > kWhole) whole(a.meta, sn.meta);
    if (cnt[Patch::EDGES] > kWhole) whole(a.edges, sn.edges);
    if (cnt[Patch::BUCKETS] > kWhole) whole(a.buckets, sn.buckets);
    if (with_reverse && cnt[Patch::RMETA] > kWhole) whole(a.rmeta, sn.rmeta);
    if (with_reverse && cnt[Patch::REDGES] > kWhole) whole(a.redges, sn.redges);
    for (const Patch &p : patches) {
        if (cnt[p.array] > kWhole && p.array != Patch::OPS) continue;
        hipError_t e1 = hipSuccess;
        switch (p.array) {
            case Patch::META: *fits = *fits && a.meta->patch(sn.meta, p.off, p.n, s, &e1); break;
            case Patch::EDGES: *fits = *fits && a.edges->patch(sn.edges, p.off, p.n, s, &e1); break;
            case Patch::BUCKETS: *fits = *fits && a.buckets->patch(sn.buckets, p.off, p.n, s, &e1); break;
            case Patch::OPS: *fits = *fits && a.ops->patch(sn.ops, p.off, p.n, s, &e1); break;
            case Patch::RMETA: if (with_reverse) *fits = *fits && a.rmeta->patch(sn.rmeta, p.off, p.n, s, &e1); break;
            case Patch::REDGES: if (with_reverse) *fits = *fits && a.redges->patch(sn.redges, p.off, p.n, s, &e1); break;
        }
        if (e1 != hipSuccess) err = e1;
    }
    return err;
}

// ---- background compaction (engine_internal.hpp Compaction); everything here runs under state_mu EXCLUSIVE except the worker
static bool compaction_due(acl_engine *h) {
    const Snapshot &s = h->snap;
    if (s.garbage_words * 8 > s.edges.size() + s.buckets.size() + h->compaction_slack) return true;  // half of the 25 % that forces a rebuild
    const Schema &sc = h->store.schema();
    // a table's spare ids running low: fewer left than a tenth of the table, or than 8 192 (half of the smallest headroom) -- the build
    // must finish before they are gone, and a small table of a fast-growing type (lock / workflow / activity ids) has no "last 10 %" to speak of
    auto low = [](uint64_t used, uint64_t cap) { return cap && used + std::max<uint64_t>(cap / 10, 8192) > cap; };
    for (int slot = 0; slot < sc.nslots && slot < (int)s.lay.size(); slot++) {
        const RelLayout &l = s.lay[slot];
        if (low(h->store.objects(sc.slot_owner[slot].first).count(), l.nrows)) return true;
        for (size_t k = 0; k < l.cls.size(); k++) {
            const auto [t, m] = sc.slot_owner[slot];
            if (l.cls[k].hashed && !sc.defs[t].members[m].classes[k].wildcard && low(h->store.objects(sc.defs[t].members[m].classes[k].stype).count(), l.cls[k].nsubjects)) return true;
        }
    }
    return false;
}

static void compaction_start(acl_engine *h) {
    if (!h->compaction_enabled || h->store_only) return;
    if (!h->compaction) h->compaction = std::make_unique<Compaction>();
    Compaction *c = h->compaction.get();
    // one at a time -- and a FINISHED build (2) waits for the next reader to adopt it: starting another one here threw it away.  That was not
    // rare: the worker's last uploads and this thread's patch upload meet in the runtime, so the build tended to finish exactly between this
    // read's adoption check and this call (4 of 5 builds were dropped in the dual-write run, and the tables ran out of spare ids meanwhile).
    if (c->state.load() == 1 || c->state.load() == 2) return;
    if (debug_rebuild()) fprintf(stderr, "[aclgpu] background build starts at revision %llu (previous state %d)\n", (unsigned long long)h->store.revision(), c->state.load());
    if (c->worker.joinable()) c->worker.join();
    // one set of fresh arrays + an upload stream per replica (created on that replica's device)
    while (c->per.size() < h->devs.size()) c->per.push_back(std::make_unique<Compaction::PerDevice>());
    for (size_t i = 0; i < h->devs.size(); i++) {
        Compaction::PerDevice &pd = *c->per[i];
        pd.device = h->devs[i]->device;
        if (!pd.stream && (hipSetDevice(pd.device) != hipSuccess || hipStreamCreateWithFlags(&pd.stream, hipStreamNonBlocking) != hipSuccess)) return;
    }
    c->now = h->store.now();
    auto view = std::make_shared<Store>(h->store.view(c->now));  // tables shared copy-on-write, expiry maps share their sorted bases: O(#tables), not O(#relationships) or O(#expiring keys)
    c->shard = h->shard;
    c->with_reverse = h->all_rev_uploaded();
    c->error.clear();
    c->state.store(1);
    const size_t ndev = h->devs.size();
    c->worker = std::thread([c, view, ndev] {
        // ONE host build, uploaded to every replica
        build_forward(*view, c->now, &c->snap, c->shard);
        if (c->with_reverse) build_reverse(*view, c->now, &c->snap, c->shard);
        const Snapshot &s = c->snap;
        bool ok = std::max({s.meta.size(), s.edges.size(), s.buckets.size()}) < ((size_t)1 << 30);
        for (size_t i = 0; ok && i < ndev; i++) {
            Compaction::PerDevice &pd = *c->per[i];
            auto up = [&](auto &dev, const auto &host) { return dev.upload(host, pd.stream) == hipSuccess; };
            ok = hipSetDevice(pd.device) == hipSuccess && up(pd.d_meta, s.meta) && up(pd.d_edges, s.edges) && up(pd.d_buckets, s.buckets) && up(pd.d_ops, s.ops) &&
                 up(pd.d_progs, s.progs) && up(pd.d_bexpr, s.bexpr) && up(pd.d_tsb, s.type_slot_base) && up(pd.d_tnm, s.type_nmembers);
            if (ok && c->with_reverse)
                ok = up(pd.d_rmeta, s.rmeta) && up(pd.d_redges, s.redges) && up(pd.d_rops, s.rops) && up(pd.d_rprogs, s.rprogs) && up(pd.d_rseeds, s.rseeds) && up(pd.d_rdest, s.rdest) &&
                     up(pd.d_sbb, s.slot_bit_base) && up(pd.d_snobj, s.slot_nobjects);
        }
        for (size_t i = 0; ok && i < ndev; i++) ok = hipSetDevice(c->per[i]->device) == hipSuccess && hipStreamSynchronize(c->per[i]->stream) == hipSuccess;
        c->state.store(ok ? 2 : 3);
    });
}

void compaction_join(acl_engine *h) {
    if (!h->compaction) return;
    if (h->compaction->worker.joinable()) h->compaction->worker.join();
    h->compaction->state.store(0);
}

static void refresh_local_blocks(acl_engine *h) {  // (the single-launch kernel's LDS depends on the schema)
    for (auto &d : h->devs) {
        d->local_blocks = local_grid_blocks(d->device, (h->snap.progs.size() + h->snap.ops.size()) * 32);
        d->local_blocks_wide = local_grid_blocks(d->device, (h->snap.progs.size() + h->snap.ops.size()) * 32, true);
    }
}

// A finished build: bring it from the view's revision to the store's with the ordinary patcher, then swap it in on every replica.
// Returns true when the engine's snapshot is now the compacted one (and current).
static bool compaction_adopt(acl_engine *h, int64_t now) {
    Compaction *c = h->compaction.get();
    if (!c || c->state.load() != 2) {
        if (c && c->state.load() == 3) {
            if (debug_rebuild()) fprintf(stderr, "[aclgpu] background build failed: %s\n", c->error.c_str());
            c->state.store(0);
        }
        return false;
    }
    c->state.store(0);
    if (c->worker.joinable()) c->worker.join();
    if (c->shard.rank != h->shard.rank || c->shard.world != h->shard.world || c->per.size() < h->devs.size()) return false;
    std::vector<Patch> patches;
    const uint64_t from = c->snap.revision;
    if (debug_rebuild()) fprintf(stderr, "[aclgpu] adopting the background build of revision %llu at revision %llu\n", (unsigned long long)from, (unsigned long long)h->store.revision());
    if (!patch_forward(h->store, now, &c->snap, h->shard, &patches, (size_t)1 << 19)) return false;  // (a bulk load meanwhile: the synchronous path decides)
    bool rev_ok = c->with_reverse && patch_reverse(h->store, now, from, &c->snap, h->shard, &patches);
    for (size_t i = 0; i < h->devs.size(); i++) {  // the catch-up patch reaches every replica's fresh arrays before any of them is swapped in
        Compaction::PerDevice &pd = *c->per[i];
        bool fits = true;
        if (hipSetDevice(pd.device) != hipSuccess) return false;
        const hipError_t pe = upload_patches(c->snap, patches, SnapArrays{&pd.d_meta, &pd.d_edges, &pd.d_buckets, &pd.d_rmeta, &pd.d_redges, &pd.d_ops}, rev_ok, h->devs[i]->up_stream, &fits);
        if (pe != hipSuccess || !fits || hipStreamSynchronize(h->devs[i]->up_stream) != hipSuccess) return false;
    }
    // swap: the old arrays go to the compaction object and are freed (or reused) by its next run
    h->set_dev_valid(false);
    h->snap = std::move(c->snap);
    c->snap = Snapshot();
    for (size_t i = 0; i < h->devs.size(); i++) {
        DevState &d = *h->devs[i];
        Compaction::PerDevice &pd = *c->per[i];
        d.d_meta.swap(pd.d_meta);
        d.d_edges.swap(pd.d_edges);
        d.d_buckets.swap(pd.d_buckets);
        d.d_ops.swap(pd.d_ops);
        d.d_progs.swap(pd.d_progs);
        d.d_bexpr.swap(pd.d_bexpr);
        d.d_tsb.swap(pd.d_tsb);
        d.d_tnm.swap(pd.d_tnm);
        if (rev_ok) {
            d.d_rmeta.swap(pd.d_rmeta);
            d.d_redges.swap(pd.d_redges);
            d.d_rops.swap(pd.d_rops);
            d.d_rprogs.swap(pd.d_rprogs);
            d.d_rseeds.swap(pd.d_rseeds);
            d.d_rdest.swap(pd.d_rdest);
            d.d_sbb.swap(pd.d_sbb);
            d.d_snobj.swap(pd.d_snobj);
        }
        d.rev_uploaded = rev_ok;
        d.dev_valid = true;
    }
    if (!rev_ok) h->snap.has_reverse = false;
    h->snap_valid = true;
    refresh_local_blocks(h);
    std::lock_guard<std::mutex> lk(h->stats_mu);
    h->stats.snapshot_compactions++;
    h->hop2_rows_now.store(h->snap.hop2_rows, std::memory_order_relaxed);
    h->stats.snapshot_edges = h->snap.nedges;
    h->stats.snapshot_edges_local = h->snap.nedges_local;
    h->stats.snapshot_bytes = h->snap.meta.size() * 4 + h->snap.edges.size() * 4 + h->snap.buckets.size() * 4 + h->snap.ops.size() * sizeof(FwdOp) +
                              h->snap.progs.size() * sizeof(SlotProg) + (rev_ok ? h->snap.rmeta.size() * 4 + h->snap.redges.size() * 4 : 0);
    return true;
}

// caller holds state_mu EXCLUSIVE: no evaluation is reading the device arrays of ANY replica.  Whatever changes the snapshot here reaches
// every replica before the function returns (DevState): an evaluation that starts afterwards answers for the store as it is now, whichever
// device it lands on -- the reference's one client is read-your-writes for the whole process (check.go:41-46, activity.go:60-77).
int ensure_snapshot(acl_engine *h) {
    if (h->store_only) return fail(ACL_ERR_UNAVAILABLE, "engine was opened store-only (no GPU): Check / LookupResources are unavailable");
    if (!h->store.has_schema()) return fail(ACL_ERR_FAILED_PRECONDITION, "no schema loaded");
    if (snapshot_current(h, false)) return ACL_OK;
    h->snap_epoch++;  // (whatever happens below changes the snapshot or fails: what was learnt about the old one -- acl_engine::deep_known -- is not carried over)
    // (schemas with `&` / `-` on a sharded graph: the snapshot builds like any other; which entry points evaluate it is ShardCall::begin's business)
    const int64_t now = h->store.now();
    if (h->snap_valid && h->all_dev_valid() && compaction_adopt(h, now) && snapshot_current(h, false)) return ACL_OK;  // a background rebuild finished: swap it in
    // a few committed writes since the snapshot: patch the rows they touch instead of rebuilding 10 M relationships
    // (... or an expiration passed: the relationships that ran out are part of the patcher's feed)
    if (h->snap_valid && h->all_dev_valid() &&
        h->snap.garbage_words * 4 < (h->snap.edges.size() + h->snap.buckets.size()) + 65536) {
        std::vector<Patch> patches;
        const uint64_t from_revision = h->snap.revision;
        if (patch_forward(h->store, now, &h->snap, h->shard, &patches)) {
            // the reverse rows (LookupResources), if they are on the devices, follow the same feed
            const bool had_rev = h->all_rev_uploaded();
            bool rev_ok = had_rev && patch_reverse(h->store, now, from_revision, &h->snap, h->shard, &patches);
            h->set_dev_valid(false);  // until every region below has reached every device
            h->set_rev_uploaded(false);
            if (std::max({h->snap.meta.size(), h->snap.edges.size(), h->snap.buckets.size()}) >= ((size_t)1 << 30))
                return fail(ACL_ERR_RESOURCE_EXHAUSTED, "snapshot array beyond 4 GiB (more than ~1 G relationships in one array): shard the graph (acl_shard_configure)");
            for (auto &dp : h->devs) {
                DevState &d = *dp;
                hipStream_t s = d.up_stream;
                HIP_TRY(hipSetDevice(d.device));
                bool fits = true;
                const hipError_t pe = upload_patches(h->snap, patches, SnapArrays{&d.d_meta, &d.d_edges, &d.d_buckets, &d.d_rmeta, &d.d_redges, &d.d_ops}, rev_ok, s, &fits);
                if (pe != hipSuccess) return fail(ACL_ERR_INTERNAL, std::string("snapshot patch upload: ") + hipGetErrorString(pe));
                if (!fits) {  // an array outgrew its device allocation: the host copy is already exact, upload it whole
                    HIP_TRY(d.d_meta.upload(h->snap.meta, s));
                    HIP_TRY(d.d_edges.upload(h->snap.edges, s));
                    HIP_TRY(d.d_buckets.upload(h->snap.buckets, s));
                    HIP_TRY(d.d_ops.upload(h->snap.ops, s));
                    if (rev_ok) {
                        HIP_TRY(d.d_rmeta.upload(h->snap.rmeta, s));
                        HIP_TRY(d.d_redges.upload(h->snap.redges, s));
                    }
                }
            }
            for (auto &dp : h->devs) {  // (the replicas' uploads overlap; one wait each)
                HIP_TRY(hipSetDevice(dp->device));
                HIP_TRY(hipStreamSynchronize(dp->up_stream));
                dp->dev_valid = true;
                dp->rev_uploaded = had_rev && rev_ok;
            }
            if (!(had_rev && rev_ok)) h->snap.has_reverse = false;  // not patchable (or never built): rebuilt lazily by the next lookup
            {
                std::lock_guard<std::mutex> lk(h->stats_mu);
                h->stats.snapshot_patches++;
                h->hop2_rows_now.store(h->snap.hop2_rows, std::memory_order_relaxed);
                h->stats.snapshot_edges = h->snap.nedges;
                h->stats.snapshot_edges_local = h->snap.nedges_local;
            }
            if (compaction_due(h)) compaction_start(h);  // garbage / headroom half used: build the next snapshot in the background
            return ACL_OK;
        }
    }
    if (debug_rebuild())
        fprintf(stderr, "[aclgpu] synchronous rebuild: snap_valid=%d dev_valid=%d window=[%lld,%lld) now=%lld garbage=%llu of %zu store_rev=%llu snap_rev=%llu\n",
                (int)h->snap_valid, (int)h->all_dev_valid(), (long long)h->snap.valid_lo, (long long)h->snap.valid_hi, (long long)now,
                (unsigned long long)h->snap.garbage_words, h->snap.edges.size() + h->snap.buckets.size(), (unsigned long long)h->store.revision(),
                (unsigned long long)h->snap.revision);
    h->snap_valid = false;
    h->set_dev_valid(false);
    h->set_rev_uploaded(false);
    build_forward(h->store, now, &h->snap, h->shard);
    h->snap_valid = true;
    // the kernels address every snapshot array as base + 32-bit byte offset (kernels.hip gld): refuse what does not fit
    if (std::max({h->snap.meta.size(), h->snap.edges.size(), h->snap.buckets.size()}) >= ((size_t)1 << 30))
        return fail(ACL_ERR_RESOURCE_EXHAUSTED, "snapshot array beyond 4 GiB (more than ~1 G relationships in one array): shard the graph (acl_shard_configure)");
    for (auto &dp : h->devs) {
        DevState &d = *dp;
        hipStream_t s = d.up_stream;
        HIP_TRY(hipSetDevice(d.device));
        HIP_TRY(d.d_meta.upload(h->snap.meta, s));
        HIP_TRY(d.d_edges.upload(h->snap.edges, s));
        HIP_TRY(d.d_buckets.upload(h->snap.buckets, s));
        HIP_TRY(d.d_ops.upload(h->snap.ops, s));
        HIP_TRY(d.d_progs.upload(h->snap.progs, s));
        HIP_TRY(d.d_bexpr.upload(h->snap.bexpr, s));
        HIP_TRY(d.d_tsb.upload(h->snap.type_slot_base, s));
        HIP_TRY(d.d_tnm.upload(h->snap.type_nmembers, s));
    }
    for (auto &dp : h->devs) {
        HIP_TRY(hipSetDevice(dp->device));
        HIP_TRY(hipStreamSynchronize(dp->up_stream));
        dp->dev_valid = true;
    }
    refresh_local_blocks(h);
    std::lock_guard<std::mutex> lk(h->stats_mu);
    h->stats.snapshot_builds++;
    h->hop2_rows_now.store(h->snap.hop2_rows, std::memory_order_relaxed);
    h->walk_no_direct.store(false, std::memory_order_relaxed);  // (a new snapshot: the direct task lists get another chance)
    h->stats.snapshot_edges = h->snap.nedges;
    h->stats.snapshot_edges_local = h->snap.nedges_local;
    h->stats.snapshot_bytes = h->snap.meta.size() * 4 + h->snap.edges.size() * 4 + h->snap.buckets.size() * 4 + h->snap.ops.size() * sizeof(FwdOp) + h->snap.progs.size() * sizeof(SlotProg);
    return ACL_OK;
}

// do the reverse rows' visited bitmaps cover every id a walk could mark?  Ids are interned without a revision bump
// (acl_intern, a lookup's subject, a LookupResources on a new object), so "same revision" does not imply it.
static bool reverse_covers(acl_engine *h) {
    const Schema &sc = h->store.schema();
    if (h->snap.slot_nobjects.size() != (size_t)sc.nslots) return false;
    for (int slot = 0; slot < sc.nslots; slot++)
        if (h->store.objects(sc.slot_owner[slot].first).count() > h->snap.slot_nobjects[slot]) return false;
    return true;
}

int ensure_reverse(acl_engine *h) {
    int rc = ensure_snapshot(h);
    if (rc) return rc;
    if (h->all_rev_uploaded() && reverse_covers(h)) return ACL_OK;
    h->set_rev_uploaded(false);
    build_reverse(h->store, h->store.now(), &h->snap, h->shard);
    for (auto &dp : h->devs) {
        DevState &d = *dp;
        hipStream_t s = d.up_stream;
        HIP_TRY(hipSetDevice(d.device));
        HIP_TRY(d.d_rmeta.upload(h->snap.rmeta, s));
        HIP_TRY(d.d_redges.upload(h->snap.redges, s));
        HIP_TRY(d.d_rops.upload(h->snap.rops, s));
        HIP_TRY(d.d_rprogs.upload(h->snap.rprogs, s));
        HIP_TRY(d.d_rseeds.upload(h->snap.rseeds, s));
        HIP_TRY(d.d_rdest.upload(h->snap.rdest, s));
        HIP_TRY(d.d_sbb.upload(h->snap.slot_bit_base, s));
        HIP_TRY(d.d_snobj.upload(h->snap.slot_nobjects, s));
    }
    for (auto &dp : h->devs) {
        HIP_TRY(hipSetDevice(dp->device));
        HIP_TRY(hipStreamSynchronize(dp->up_stream));
        dp->rev_uploaded = true;
    }
    std::lock_guard<std::mutex> lk(h->stats_mu);
    h->stats.snapshot_bytes += h->snap.rmeta.size() * 4 + h->snap.redges.size() * 4;
    return ACL_OK;
}

// device ordinal a device pointer lives on (-1: one replica, or not a device pointer: any replica will do)
int device_of(acl_engine *h, const void *p) {
    if (h->devs.size() < 2 || !p) return -1;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    return a.device;
}

int Eval::begin(acl_engine *h_, bool need_reverse, const CallOpts &opts, int rev_key_slot, int on_device, bool need_subjects, const std::vector<int> *more_key_slots) {
    h = h_;
    if (h->store_only) return fail(ACL_ERR_UNAVAILABLE, "engine was opened store-only (no GPU): Check / LookupResources are unavailable");
    int rc = check_opts(opts);
    if (rc) return rc;
    for (;;) {
        h->state_mu.lock_shared();
        bool ok = snapshot_current(h, need_reverse);
        // a `type#relation` lookup subject is itself a state of the walk: its id must lie inside the visited bitmap
        const auto key_slot_covered = [&](int slot) { return h->store.objects(h->store.schema().slot_owner[slot].first).count() <= h->snap.slot_nobjects[slot]; };
        if (ok && need_reverse && rev_key_slot >= 0 && !key_slot_covered(rev_key_slot)) ok = false;
        if (ok && need_reverse && more_key_slots)
            for (int slot : *more_key_slots)
                if (slot >= 0 && !key_slot_covered(slot)) ok = false;
        if (ok && need_subjects && !subjects_current(h)) ok = false;
        if (ok) {
            locked = true;
            break;
        }
        h->state_mu.unlock_shared();
        std::lock_guard<RwLock> lk(h->state_mu);
        rc = need_reverse ? ensure_reverse(h) : ensure_snapshot(h);
        if (rc == ACL_OK && need_subjects) rc = ensure_subjects(h);
        if (rc) return rc;
    }
    // a context from the pool (created on demand up to max_ctx per replica)
    std::unique_lock<std::mutex> lk(h->pool_mu);
    for (;;) {
        // Replicas (engines opened on several devices): the least loaded one that can serve the call -- ties go round the devices, so N
        // blocking callers end up on N devices.  Within a replica: the context released last (its buffers are the warmest).
        DevState *bd = nullptr;
        int bpick = -1;
        bool bcreate = false;
        const size_t nd = h->devs.size(), d0 = nd > 1 ? h->next_dev++ % nd : 0;
        for (size_t k = 0; k < nd; k++) {
            DevState *d = h->devs[(d0 + k) % nd].get();
            if (on_device >= 0 && d->device != on_device) continue;
            const int pick = d->free_ctxs.empty() ? -1 : (int)d->free_ctxs.size() - 1;  // (the one released last: its buffers are the warmest)
            const bool may_create = d->ctxs.size() < h->max_ctx;
            const bool take = pick >= 0;
            if (!take && !may_create) continue;
            if (!bd || d->in_use < bd->in_use) {
                bd = d;
                bpick = take ? pick : -1;
                bcreate = !take;
            }
        }
        if (bd && !bcreate) {
            c = bd->free_ctxs[bpick];
            bd->free_ctxs.erase(bd->free_ctxs.begin() + bpick);
            bd->in_use++;
            bd->calls++;
            break;
        }
        if (bd) {
            std::unique_ptr<PassCtx> nc;
            rc = new_ctx(h, bd, &nc, (int)bd->ctxs.size());
            if (rc) return rc;
            c = nc.get();
            bd->ctxs.push_back(std::move(nc));
            bd->in_use++;
            bd->calls++;
            break;
        }
        if (on_device >= 0) {
            bool any = false;
            for (auto &d : h->devs) any = any || d->device == on_device;
            if (!any) return fail(ACL_ERR_INVALID_ARGUMENT, "the device buffers live on a device this engine holds no replica on");
        }
        if (opts.cancel || opts.deadline_ns) {
            h->pool_cv.wait_for(lk, std::chrono::microseconds(500));
            rc = check_opts(opts);
            if (rc) return rc;
        } else {
            h->pool_cv.wait(lk);
        }
    }
    lk.unlock();
    // everything this call allocates, copies and launches happens on the context's device
    HIP_TRY(hipSetDevice(c->dev->device));
    c->opts = opts;
    c->timing = h->timing.load(std::memory_order_relaxed);
    return ACL_OK;
}

void Eval::end() {
    if (c) {
        merge_stats(h, c);
        c->opts = CallOpts();
        {
            std::lock_guard<std::mutex> lk(h->pool_mu);
            c->dev->free_ctxs.push_back(c);
            c->dev->in_use--;
        }
        // every waiter: one that asked for a replica on a particular device cannot use a context of another one, and a wake-up it consumed
        // would leave a second waiter asleep next to a free context
        h->pool_cv.notify_all();
        c = nullptr;
    }
    if (locked) {
        h->state_mu.unlock_shared();
        locked = false;
    }
}

}  // namespace aclint

// engine_pass.cpp -- the forward passes: evaluation contexts (PassCtx) and their timing events, the single-launch walk
// (k_check_local) over device or host-mapped batches, the level loop it falls back to, and the id entry points' host half.
#include "engine_internal.hpp"

namespace aclint {

thread_local std::string g_last_error;
thread_local int g_last_detail = 0;

int64_t mono_ns() { return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int check_opts(const CallOpts &o) {
    if (o.cancel && *o.cancel) return fail(ACL_ERR_CANCELLED, "call cancelled by the caller");
    if (o.deadline_ns && mono_ns() >= o.deadline_ns) return fail(ACL_ERR_DEADLINE_EXCEEDED, "deadline exceeded");
    return ACL_OK;
}

PassCtx::~PassCtx() {
    if (stream) (void)hipStreamSynchronize(stream);
    for (hipStream_t a : aux)
        if (a) {
            (void)hipStreamSynchronize(a);
            (void)hipStreamDestroy(a);
        }
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    if (h_status) (void)hipHostFree(h_status);
    if (stream) (void)hipStreamDestroy(stream);
}

int alloc_frontier(acl_engine *h, PassCtx *c, uint64_t entries) {
    // every wave of an expand launch owns one static chunk; at least one dynamic chunk on top
    entries = std::max<uint64_t>(entries, ((uint64_t)c->dev->grid_blocks * kWavesPerBlock + 1) * kChunk);
    uint64_t chunks = (entries + kChunk - 1) / kChunk;
    if (chunks > kMaxFrontierChunks) chunks = kMaxFrontierChunks;  // byte offsets of entries stay below 2^32 (kernels.hip gld / gst)
    for (int i = 0; i < 2; i++) {
        c->d_fbuf[i].release();
        c->d_fcounts[i].release();
        HIP_TRY(c->d_fbuf[i].ensure(chunks * kChunk));
        HIP_TRY(c->d_fcounts[i].ensure(chunks));
    }
    c->max_chunks = (uint32_t)chunks;
    c->frontier_entries = chunks * kChunk;
    return ACL_OK;
}

int new_ctx(acl_engine *h, DevState *d, std::unique_ptr<PassCtx> *out, int index) {
    HIP_TRY(hipSetDevice(d->device));
    auto c = std::make_unique<PassCtx>();
    c->index = index;
    c->dev = d;
    HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIP_TRY(c->d_status.ensure(kStatusWords));
    HIP_TRY(c->d_done.ensure(1));
    HIP_TRY(hipMemset(c->d_done.p, 0, sizeof(uint32_t)));
    HIP_TRY(hipHostMalloc((void **)&c->h_status, kStatusWords * sizeof(uint32_t), hipHostMallocDefault));
    int rc = alloc_frontier(h, c.get(),
                            h->cfg_frontier_entries ? h->cfg_frontier_entries : std::max<uint64_t>(32u << 20, (uint64_t)2 * d->grid_blocks * kWavesPerBlock * kChunk));  // 2 x 512 MiB: the single-launch walk carves its blocks' private regions out of these
    if (rc) return rc;
    *out = std::move(c);
    return ACL_OK;
}

// ---- timing helpers: one HIP event pair per kernel launch, on the context's stream
void ev_begin(PassCtx *c, int kind) {
    if (!c->timing) return;
    if (c->ev_used + 2 > c->ev.size()) {
        for (int i = 0; i < 2; i++) {
            hipEvent_t e;
            (void)hipEventCreate(&e);
            c->ev.push_back(e);
        }
        c->ev_kind.push_back(0);
    }
    c->ev_kind[c->ev_used / 2] = kind;
    (void)hipEventRecord(c->ev[c->ev_used], c->stream);
}
void ev_end(PassCtx *c) {
    if (!c->timing) return;
    (void)hipEventRecord(c->ev[c->ev_used + 1], c->stream);
    c->ev_used += 2;
}
void ev_collect(PassCtx *c) {  // stream must be synchronized
    for (size_t i = 0; i + 1 < c->ev_used; i += 2) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, c->ev[i], c->ev[i + 1]) == hipSuccess) {
            c->stats.kernel_ms += ms;
            if (c->ev_kind[i / 2] == 1) c->stats.expand_ms += ms;
            else if (c->ev_kind[i / 2] == 2) c->stats.local_ms += ms;
            else if (c->ev_kind[i / 2] == 3) c->stats.rev_local_ms += ms;
            else if (c->ev_kind[i / 2] == 4) c->stats.subj_local_ms += ms;
            else if (c->ev_kind[i / 2] == 5) c->stats.refine_ms += ms;
            else if (c->ev_kind[i / 2] == 6) c->stats.rev_multi_ms += ms;
        }
    }
    c->ev_used = 0;
}

void merge_stats(acl_engine *h, PassCtx *c) {
    std::lock_guard<std::mutex> lk(h->stats_mu);
    acl_stats_t &a = h->stats, &b = c->stats;
    a.check_items += b.check_items;
    a.check_passes += b.check_passes;
    a.expand_launches += b.expand_launches;
    if (b.check_passes || b.lookup_requests) a.levels_last = b.levels_last;
    a.frontier_entries += b.frontier_entries;
    a.kernel_ms += b.kernel_ms;
    a.expand_ms += b.expand_ms;
    a.local_ms += b.local_ms;
    a.local_passes += b.local_passes;
    a.rev_local_ms += b.rev_local_ms;
    a.rev_local_passes += b.rev_local_passes;
    a.subj_local_ms += b.subj_local_ms;
    a.refine_ms += b.refine_ms;
    a.rev_multi_ms += b.rev_multi_ms;
    a.rev_multi_passes += b.rev_multi_passes;
    a.lookup_requests += b.lookup_requests;
    a.overflow_retries += b.overflow_retries;
    b = acl_stats_t{};
}



// Small batches: the kernel's last block stores `val` into a pinned word behind a system-scope release of everything the launch wrote into host
// memory; the caller spins on that word instead of entering hipStreamSynchronize, which returns ~5.5 us after the store is visible
// (tools/launch_latency.hip).  false: the word did not arrive within 2 ms (a fault, a debugger) -- the caller falls back to the synchronising wait,
// which reports the error.  The stream is left un-synchronised on purpose: everything else on it is ordered behind the kernel anyway.
bool spin_for(const volatile uint32_t *word, uint32_t val) {
    const int64_t t_end = mono_ns() + 2000000;
    for (uint32_t it = 0;; it++) {
        if (*word == val) {
            std::atomic_thread_fence(std::memory_order_acquire);
            return true;
        }
        if ((it & 1023u) == 1023u && mono_ns() > t_end) return false;
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
}
uint32_t next_done_val(PassCtx *c) {
    uint32_t v = ++c->done_seq;
    if (!v) v = c->done_seq = 1;  // (0 never names a launch)
    return v;
}

// Small batch: ONE launch (k_check_local) seeds, walks every level and writes the answers.  Requests per wave: one while the
// batch fits the chip's wave slots (latency), more beyond that.  The waves' private frontier regions are carved from
// the context's frontier buffers.
constexpr uint32_t kLocalWideMin = 65536;  // batches from this size on run the wide (12-wave) instantiation: a unit pools more requests, shorter tail (profiles/r03_wide_threshold.txt)
constexpr uint32_t kHostSkewPct = 8;  // a lone caller's host-mapped launch: first unit this many percent larger than the mean, last one as much smaller (profiles/r04_host_skew.txt)
// Geometry of a single-launch pass over n requests: requests per unit, blocks to launch, private frontier entries per block.
struct LocalGeom {
    uint32_t rpw, nblocks, nunits, cap;
    bool wide = false;  // 12 waves per block and unit (kLocalWide) (chip-filling batches) instead of 4
};
static LocalGeom local_geom(acl_engine *h, PassCtx *c, uint32_t n) {
    LocalGeom G{};
    G.wide = n >= kLocalWideMin;
    const uint32_t blocks = (uint32_t)(G.wide ? c->dev->local_blocks_wide : c->dev->local_blocks);  // what is resident at once; a unit is walked by one block (4 or 12 waves)
    // latency: while the batch has fewer requests than the chip has blocks, every request gets a block of its own; beyond that
    // every block gets ONE unit of n / blocks requests (profiles/r02_walk_units_per_wave.txt, profiles/r03_static_dynamic_units_ab.txt)
    G.rpw = n <= blocks ? 1u : std::min<uint32_t>(std::max<uint32_t>((n + blocks - 1) / blocks, 1), local_unit_max(G.wide));
    G.nunits = (n + G.rpw - 1) / G.rpw;
    G.nblocks = std::max<uint32_t>(std::min<uint32_t>(G.nunits, blocks), 1);
    // (a block that needs more than 256 K entries is walking something the whole chip should walk: the level loop takes the batch)
    G.cap = (uint32_t)std::min<uint64_t>(c->frontier_entries / G.nblocks, 1u << 18);
    if (h->local_cap_limit) G.cap = std::min(G.cap, h->local_cap_limit);
    return G;
}

int combine_prepare(acl_engine *h, PassCtx *c, DevGraph *g, uint32_t n, uint32_t blocks, uint32_t rpw) {
    if (!h->snap.has_combine) return ACL_OK;
    // nodes: one per visited state with a combine program; cells: its leaves (<= kMaxLeaves, typically 2-3).  A block of the single-launch walk
    // that outgrows its share sends the batch to the level loop; the level loop's pool running out fails the call.
    uint64_t node_cap, regions = 1;
    if (blocks) {
        node_cap = std::max<uint64_t>(1024, (uint64_t)rpw * 8);
        regions = blocks;
    } else {
        node_cap = std::min<uint64_t>(std::max<uint64_t>((uint64_t)1 << 20, (uint64_t)n * 16) << c->pool_shift, (uint64_t)1 << 26);
    }
    const uint64_t cell_cap = node_cap * 4;
    if ((uint64_t)n + regions * cell_cap >= 0xFFFFFFF0ull) return fail(ACL_ERR_RESOURCE_EXHAUSTED, "combine cells beyond 2^32: lower max_sub_batch");
    HIP_TRY(c->d_nodes.ensure(regions * node_cap));
    HIP_TRY(c->d_has.ensure((size_t)n + regions * cell_cap));
    HIP_TRY(c->d_err.ensure((size_t)n + regions * cell_cap));
    g->bexpr = c->dev->d_bexpr.p;
    g->nodes = c->d_nodes.p;
    g->node_cap = (uint32_t)node_cap;
    g->cell_cap = (uint32_t)cell_cap;
    g->cell0 = n;
    g->ccount = blocks ? nullptr : c->d_status.p + 2 * kLevelSlots + 2;  // (the per-destination export counters of the sharded walk: unused here, reset by k_seed)
    return ACL_OK;
}

// enqueue-only half (memset of the flag, the launch, the flag's read-back)
static int local_enqueue(acl_engine *h, PassCtx *c, const DevGraph &g0, const uint4 *d_items, uint32_t n, uint8_t *d_perm, int32_t *d_errout) {
    const LocalGeom G = local_geom(h, c, n);
    if (G.cap < 256) return kTakeLevelLoop;
    DevGraph g = g0;
    if (int rc = combine_prepare(h, c, &g, n, G.nblocks, G.rpw)) return rc;
    uint32_t *d_over = c->d_status.p + 2 * kLevelSlots;  // [0] overflow flag, [1] next unit (the sharded walk's export counter: unused here)
    HIP_TRY(hipMemsetAsync(d_over, 0, 3 * sizeof(uint32_t), c->stream));  // [2]: deepest level (a per-destination export counter of the sharded walk: unused here)
    ev_begin(c, 2);
    launch_check_local(c->stream, g, d_items, n, G.rpw, G.nblocks, G.nunits > G.nblocks ? d_over + 1 : nullptr, c->d_fbuf[0].p, c->d_fbuf[1].p, G.cap, d_over, c->d_has.p,
                       c->d_err.p, d_perm, d_errout, d_over + 2, G.wide);
    ev_end(c);
    HIP_TRY(hipMemcpyAsync(c->h_status, d_over, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    return ACL_OK;
}
static int local_finish(acl_engine *h, PassCtx *c, uint32_t n) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    ev_collect(c);
    if (c->h_status[0] == 2) return fail(ACL_ERR_RESOURCE_EXHAUSTED, "a relationship row exceeds the per-task enumeration limit");
    if (c->h_status[0] == kOverflowDirect) {
        h->walk_no_direct.store(true, std::memory_order_relaxed);
        c->direct_tripped = true;
    }
    if (c->h_status[0]) return kTakeLevelLoop;
    c->stats.levels_last = c->h_status[2];
    c->stats.check_items += n;
    c->stats.check_passes++;
    c->stats.local_passes++;
    return ACL_OK;
}
int check_pass_local(acl_engine *h, PassCtx *c, const DevGraph &g, const uint4 *d_items, uint32_t n, uint8_t *d_perm, int32_t *d_errout) {
    const int rc = local_enqueue(h, c, g, d_items, n, d_perm, d_errout);
    return rc ? rc : local_finish(h, c, n);
}

static bool walk_allowed(acl_engine *h, size_t n);
static void walk_outcome(acl_engine *h, PassCtx *c, size_t n, int rc);

// The same for a batch in HOST memory, with no copy engine in the path: the kernel reads the items from pinned host memory
// and writes the answers (and its overflow flag) straight back into pinned host memory, so a pass is ONE launch and ONE
// stream synchronisation -- no H2D, no flag memset, no D2H copies, each of which costs a few microseconds of API time that a
// 64-item batch cannot amortise.  Returns ACL_ERR_RESOURCE_EXHAUSTED (quietly) when the batch must take the level loop.
static int check_pass_local_host(acl_engine *h, PassCtx *c, const acl_item_t *items, uint32_t n, uint8_t *perm_out, int32_t *err_out, bool *attempted) {
    *attempted = false;
    // A batch beyond what one launch takes with one unit per resident block (524 288 items on this chip) goes as SUB-PASSES of equal size: one
    // launch each, back to back on the context's stream, every one reading its slice of the items from -- and answering into -- the caller's
    // pinned memory, ONE synchronisation for all (round 4: this retired the copying pipeline -- look-ahead H2D, lanes, kernels chained on the
    // device through events, a completer thread -- that served only such batches).
    const bool wide0 = n >= kLocalWideMin;
    const uint64_t per_launch = (uint64_t)(wide0 ? c->dev->local_blocks_wide : c->dev->local_blocks) * local_unit_max(wide0);
    uint32_t npass = (uint32_t)std::max<uint64_t>(1, ((uint64_t)n + per_launch - 1) / per_launch);
    // CONCURRENT slices: the items of a launch cross PCIe while its blocks wait for their seeds (4 MB per 262 144 items: ~80 us in which a lone
    // caller's chip idles).  On two streams, the first slice's blocks fill the chip and compute while the second slice's blocks -- which move in
    // as those finish -- fetch theirs; each stream walks in a frontier region of its own.  Sub-passes of a batch beyond one launch always
    // alternate between the two streams (1 048 576 items from one caller: 800 -> 933 M decisions/s); a batch that fits one launch is cut in two
    // only for a LONE caller and only from 262 144 items on (0.336 -> 0.324 ms): the halves' units are half as long, which costs three concurrent
    // callers a tenth of their throughput, and three or four slices lose outright (profiles/r04_host_split.txt).  Not with combine schemas (the
    // slices would share the node / cell scratch) and not while kernels are being timed (the events sit on the context's stream).
    uint32_t nstreams = 1;
    bool lone = false;
    if (n >= 65536) {
        std::lock_guard<std::mutex> lk(h->pool_mu);
        lone = c->dev->in_use <= 1;
    }
    const bool lone_split = lone && npass == 1 && n >= 262144;
    if (h->host_split > 1 && !h->snap.has_combine && !c->timing && (npass > 1 || lone_split)) {
        nstreams = std::min<uint32_t>(h->host_split, 4);
        npass = std::max(npass, nstreams);
    }
    const uint32_t chunk = npass == 1 ? n : (uint32_t)((((uint64_t)n + npass - 1) / npass + 63) / 64 * 64);
    LocalGeom G = local_geom(h, c, std::min(n, chunk));
    G.cap /= nstreams;
    if (G.cap < 256 || G.nunits > G.nblocks || npass > 15) return kTakeLevelLoop;
    for (uint32_t k = 1; k < nstreams; k++)
        if (!c->aux[k - 1]) HIP_TRY(hipStreamCreateWithFlags(&c->aux[k - 1], hipStreamNonBlocking));
    *attempted = true;
    HIP_TRY(c->d_has.ensure(std::max<size_t>(n, 4096)));
    HIP_TRY(c->d_err.ensure(std::max<size_t>(n, 4096)));
    // the caller's own buffers where they are pinned (acl_host_alloc), else the context's pinned staging
    const void *src = items;
    if ((const void *)items != c->h_in.p && !h->is_pinned(items, (size_t)n * sizeof(acl_item_t))) {
        HIP_TRY(c->h_in.ensure((size_t)n * sizeof(acl_item_t)));
        std::memcpy(c->h_in.p, items, (size_t)n * sizeof(acl_item_t));
        src = c->h_in.p;
    }
    const bool pin_p = h->is_pinned(perm_out, n), pin_e = err_out && h->is_pinned(err_out, (size_t)n * sizeof(int32_t));
    HIP_TRY(c->h_out.ensure(64 + (size_t)n * 5));
    uint32_t *flag = (uint32_t *)c->h_out.p;  // one overflow flag per sub-pass (16 words)
    int32_t *h_err = pin_e ? err_out : (int32_t *)((char *)c->h_out.p + 64);
    uint8_t *h_perm = pin_p ? perm_out : (uint8_t *)c->h_out.p + 64 + (size_t)n * 4;
    std::memset(flag, 0, 64);  // (word 15: the completion word of small batches)
    const bool spin = npass == 1 && nstreams == 1 && !c->timing && n <= h->spin_max && !h->snap.has_combine;
    const uint32_t done_val = spin ? next_done_val(c) : 0u;
    void *d_in = nullptr, *d_flag = nullptr, *d_perm = nullptr, *d_errp = nullptr;
    // (the staging buffers' device pointers are kept with them; only a caller's own pinned buffer is asked for)
    if (src == c->h_in.p) d_in = c->h_in.dp;
    else HIP_TRY(hipHostGetDevicePointer(&d_in, const_cast<void *>(src), 0));
    d_flag = c->h_out.dp;
    if (pin_p) HIP_TRY(hipHostGetDevicePointer(&d_perm, h_perm, 0));
    else d_perm = (char *)c->h_out.dp + ((char *)h_perm - (char *)c->h_out.p);
    if (pin_e) HIP_TRY(hipHostGetDevicePointer(&d_errp, h_err, 0));
    else d_errp = (char *)c->h_out.dp + ((char *)h_err - (char *)c->h_out.p);
    // (No turn-taking between callers here, whatever the batch size: two single-launch kernels on the chip at once do not get in each other's
    //  way -- the second one's blocks move in as the first one's finish, which fills the tail a lone launch leaves idle: 2 / 4 / 8 / 16 callers
    //  with 262 144-item batches measure 886 / 890 / 914 / 916 M decisions/s, ABOVE the 873 M/s of back-to-back device-resident launches, and a
    //  host mutex around launch + synchronise costs a third of that; profiles/r03_hostmapped_batches.txt.)
    DevGraph g = h->dev_graph(c);
    if (int rc = combine_prepare(h, c, &g, std::min(n, chunk), G.nblocks, G.rpw)) return rc;  // (the sub-passes follow each other on one stream: they share the scratch)
    for (uint32_t k = 0; k < npass; k++) {
        const uint32_t off = k * chunk, m = std::min(chunk, n - off);
        LocalGeom Gk = G;
        if (k + 1 == npass && npass > 1 && m != chunk) {  // (the last one may be shorter)
            Gk = local_geom(h, c, m);
            Gk.cap = std::min(G.cap, Gk.cap);
        }
        const uint32_t lane = k % nstreams;  // slices of one lane follow each other on its stream and share its frontier region
        const size_t region = (size_t)lane * (c->frontier_entries / nstreams);
        hipStream_t st = lane ? c->aux[lane - 1] : c->stream;
        if (nstreams == 1) ev_begin(c, 2);
        launch_check_local(st, g, (const uint4 *)d_in + off, m, Gk.rpw, Gk.nblocks, nullptr, c->d_fbuf[0].p + region, c->d_fbuf[1].p + region, Gk.cap, (uint32_t *)d_flag + k,
                           c->d_has.p + off, c->d_err.p + off, (uint8_t *)d_perm + off, (int32_t *)d_errp + off, nullptr, Gk.wide,
                           lone && Gk.nunits > 1 ? Gk.rpw * kHostSkewPct / 100 : 0u, spin ? c->d_done.p : nullptr, spin ? (uint32_t *)d_flag + 15 : nullptr, done_val,
                           npass == 1 && n <= 4 ? (const uint4 *)items : nullptr);
        if (nstreams == 1) ev_end(c);
    }
    const bool spun = spin && spin_for(flag + 15, done_val);  // (small batches: see spin_for)
    if (!spun) HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t k = 1; k < nstreams; k++) HIP_TRY(hipStreamSynchronize(c->aux[k - 1]));
    ev_collect(c);
    for (uint32_t k = 0; k < npass; k++)
        if (flag[k] == 2) return fail(ACL_ERR_RESOURCE_EXHAUSTED, "a relationship row exceeds the per-task enumeration limit");
    for (uint32_t k = 0; k < npass; k++)
        if (flag[k] == kOverflowDirect) {
            h->walk_no_direct.store(true, std::memory_order_relaxed);
            c->direct_tripped = true;
        }
    for (uint32_t k = 0; k < npass; k++)
        if (flag[k]) return kTakeLevelLoop;
    if (!pin_p) std::memcpy(perm_out, h_perm, n);
    if (err_out && !pin_e) std::memcpy(err_out, h_err, (size_t)n * sizeof(int32_t));
    c->stats.check_items += n;
    c->stats.check_passes += npass;
    c->stats.local_passes += npass;
    return ACL_OK;
}

// would check_pass_local_host take a batch of n items?  (what the submit pipeline asks before it decides who runs a ticket)
bool hostmap_takes(acl_engine *h, size_t n) {
    if (!(n <= h->local_max_items && n <= h->max_sub_batch && h->shard.world == 1)) return false;
    const bool wide = n >= kLocalWideMin;
    return n <= 15 * (uint64_t)(wide ? h->dev0().local_blocks_wide : h->dev0().local_blocks) * local_unit_max(wide);  // (up to 15 sub-passes of one unit per resident block; replicas are alike)
}

// A graph whose walks keep outgrowing the blocks' private regions should not pay for a failed walk before every level loop: after an
// overflow the walk sits out 2, 4, ... 64 large passes before it is tried again.
static bool walk_allowed(acl_engine *h, size_t n) {
    if (n < kComputeTokenItems) return true;
    return !(h->local_skip.load(std::memory_order_relaxed) > 0 && h->local_skip.fetch_sub(1, std::memory_order_relaxed) > 0);
}
static void walk_outcome(acl_engine *h, PassCtx *c, size_t n, int rc) {
    // (what THIS call's walk met, kept in its own context: an engine-wide flag let two concurrent callers swap outcomes -- ADVICE r5)
    const bool direct = c->direct_tripped;
    c->direct_tripped = false;
    if (n < kComputeTokenItems) return;
    if (rc == kTakeLevelLoop && direct) return;  // (not a frontier overflow: the next walk simply builds its task lists the general way)
    if (rc == kTakeLevelLoop) h->local_skip.store(1 << std::min(6, 1 + h->local_fail_streak.fetch_add(1, std::memory_order_relaxed)), std::memory_order_relaxed);
    else if (!rc) h->local_fail_streak.store(0, std::memory_order_relaxed);
}

// the level-synchronous pass (one k_expand launch per dispatch level); `merging`: duplicate entries are struck after every level
static int levels_pass(acl_engine *h, PassCtx *c, const DevGraph &g0, const uint4 *d_items, uint32_t n, uint8_t *d_perm, int32_t *d_errout, bool merging_asked) {
    // Schemas with `&` / `-`: entries carry result CELLS where the request would be; duplicates are merged on (cell, state, level) through a
    // two-part key (k_dedup_cells), before the duplicate could create a combine node of its own; the combine nodes are evaluated behind the
    // last level, before the answers are written.
    const bool combine = h->snap.has_combine, merging = merging_asked;
    DevGraph g = g0;
    if (int rc = combine_prepare(h, c, &g, n, 0, 0)) return rc;
    for (int attempt = 0;; attempt++) {
        if ((uint64_t)n > c->frontier_entries) {
            int rc = alloc_frontier(h, c, (uint64_t)n * 4);
            if (rc) return rc;
        }
        uint32_t bits = 0;
        if (merging) {
            int rc = dedup_table(c, combine, &bits);
            if (rc) return rc;
        }
        DevFrontier f = h->dev_frontier(*c);
        ev_begin(c, 0);
        launch_seed(c->stream, g, f, d_items, n, c->d_has.p, c->d_err.p);  // also resets the status block
        ev_end(c);
        uint32_t levels = 0;
        int rc = level_loop(
            h, c, kMaxLevels,
            [&](uint32_t it) {
                launch_expand(c->stream, g, f, it, c->d_has.p, c->d_err.p);
                if (merging) launch_dedup(c->stream, f, it, c->d_dedup.p, bits, combine);
            },
            &levels,
            [&] {
                if (combine) return;  // (no speculative epilogue: a cell read before its walk is over would turn `a - b` true for good)
                ev_begin(c, 0);
                launch_finalize(c->stream, n, c->d_has.p, c->d_err.p, d_perm, d_errout);
                ev_end(c);
            });
        if (!rc && combine) {
            for (uint32_t it = levels + 1; it >= 1; it--) launch_resolve(c->stream, g, it, c->d_has.p, c->d_err.p);
            launch_finalize(c->stream, n, c->d_has.p, c->d_err.p, d_perm, d_errout);
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
        // (combine schemas: a pass that ran out of nodes / cells is first redone with duplicates merged as well -- on a cyclic graph every
        //  repeated visit of a non-monotone state was about to create a node of its own)
        if (rc == ACL_ERR_RESOURCE_EXHAUSTED && combine && !merging_asked && c->h_status[2 * kLevelSlots] == 3) return kRetryMerging;
        if (rc == ACL_ERR_RESOURCE_EXHAUSTED && c->h_status[2 * kLevelSlots] == 1) {
            if (!merging_asked) return kRetryMerging;
            // out of chunks even with duplicates merged: grow (up to 2^28 entries) and redo the pass
            c->stats.overflow_retries++;
            if (c->frontier_entries >= (uint64_t)kMaxFrontierChunks * kChunk || attempt > 8)
                return fail(ACL_ERR_RESOURCE_EXHAUSTED, "frontier capacity exceeded (" + std::to_string(c->frontier_entries) + " entries); lower max_sub_batch");
            int rc2 = alloc_frontier(h, c, c->frontier_entries * 4);
            if (rc2) return rc2;
            continue;
        }
        if (rc) return rc;
        c->levels_hint = levels;
        c->stats.levels_last = levels;
        c->stats.check_items += n;
        c->stats.check_passes++;
        return ACL_OK;
    }
}

// A merging pass over a slice whose combine nodes outgrow the pool (2^20 nodes, or 16 per item) is redone on the slice's halves: what runs out may be
// the SUM of the items' nodes -- chains of cycles through permissions with `&` / `-`, or the many paths of an acyclic graph, cost thousands of nodes an
// item (found by the random schemas of tests/schema_gen.py) -- which the oracles answer item by item.  A slice of at most kBigPoolItems items that
// still runs out is redone with a pool of 2^24 nodes, and halved again under that pool down to one item.  An item that outgrows 2^24 nodes alone fails
// the call; it has then been walked about 2 log2(n) times on the way down, and every failed attempt leaves its text as the last error until the call
// returns.  Only this path halves: the sharded native loops and the passes of the other walks keep their one pool per pass.
constexpr uint32_t kBigPoolItems = 64, kBigPoolShift = 4;
static int levels_pass_merging(acl_engine *h, PassCtx *c, const DevGraph &g, const uint4 *d_items, uint32_t n, uint8_t *d_perm, int32_t *d_errout, uint32_t shift = 0) {
    c->pool_shift = shift;
    int rc = levels_pass(h, c, g, d_items, n, d_perm, d_errout, true);
    c->pool_shift = 0;
    if (rc != ACL_ERR_RESOURCE_EXHAUSTED || !h->snap.has_combine || c->h_status[2 * kLevelSlots] != 3) return rc;
    if (n <= kBigPoolItems && shift == 0) return levels_pass_merging(h, c, g, d_items, n, d_perm, d_errout, kBigPoolShift);
    if (n == 1) return rc;
    const uint32_t half = n / 2;
    rc = levels_pass_merging(h, c, g, d_items, half, d_perm, d_errout, shift);
    if (rc) return rc;
    return levels_pass_merging(h, c, g, d_items + half, n - half, d_perm + half, d_errout ? d_errout + half : nullptr, shift);
}

// one device pass over n (<= max_sub_batch) interned items already in HBM
int check_pass(acl_engine *h, PassCtx *c, const uint4 *d_items, uint32_t n, uint8_t *d_perm, int32_t *d_errout, bool try_local) {
    HIP_TRY(c->d_has.ensure(std::max<size_t>(n, 4096)));
    HIP_TRY(c->d_err.ensure(std::max<size_t>(n, 4096)));
    DevGraph g = h->dev_graph(c);
    // small batches (the proxy's own call shape: check.go:76-94, watch.go:50): ONE launch runs every level, each wave
    // walking its own slice of the batch through a wave-private frontier -- no host round trip between levels
    if (try_local && n <= h->local_max_items && walk_allowed(h, n)) {
        int rc = check_pass_local(h, c, g, d_items, n, d_perm, d_errout);
        walk_outcome(h, c, n, rc);
        if (rc != kTakeLevelLoop) return rc;  // kTakeLevelLoop: a block ran out of private frontier, the level-synchronous path takes the batch
    }
    int rc = levels_pass(h, c, g, d_items, n, d_perm, d_errout, false);
    if (rc != kRetryMerging) return rc;
    // The frontier outgrew its buffers.  Before growing them: merge identical (request, state, level) entries after every level
    // (k_dedup) -- nested groups with branching cycles double the frontier per level otherwise -- on slices the dedup key can hold.
    c->stats.overflow_retries++;
    for (uint32_t off = 0; off < n; off += kDedupBatch) {
        const uint32_t m = std::min<uint32_t>(kDedupBatch, n - off);
        rc = levels_pass_merging(h, c, g, d_items + off, m, d_perm + off, d_errout ? d_errout + off : nullptr);
        if (rc) return rc;
    }
    return ACL_OK;
}

int not_sharded(acl_engine *h) {
    if (h->shard.world > 1)
        return fail(ACL_ERR_FAILED_PRECONDITION, "this engine holds one shard of the graph: evaluate through acl_shard_* with the other shards");
    return ACL_OK;
}

int check_device(acl_engine *h, PassCtx *c, const uint4 *d_items, size_t n, uint8_t *d_perm, int32_t *d_errout, bool try_local) {
    int rc = not_sharded(h);
    if (rc) return rc;
    for (size_t b = 0; b < n; b += h->max_sub_batch) {
        uint32_t m = (uint32_t)std::min<size_t>(h->max_sub_batch, n - b);
        rc = check_pass(h, c, d_items + b, m, d_perm + b, d_errout ? d_errout + b : nullptr, try_local);
        if (rc) return rc;
    }
    return ACL_OK;
}

// Host items in, host answers out (SURVEY.md 8(d) timing variant (ii)): H2D, kernels, D2H on the context's stream.
// Buffers from acl_host_alloc are pinned and are DMA'd directly; anything else is staged through the context's pinned
// buffers (an async copy from pageable memory would be staged by the runtime anyway, synchronously).
int check_ids_host(acl_engine *h, PassCtx *c, const acl_item_t *items, size_t n, uint8_t *perm_out, int32_t *err_out, bool items_on_device) {
    const bool walk = n <= h->local_max_items && n <= h->max_sub_batch && h->shard.world == 1;
    const bool allowed = walk && walk_allowed(h, n);  // (asked once per call: it counts down the back-off after an overflow)
    bool tried = false;  // the single-launch walk has had its go at this batch
    if (allowed && !items_on_device) {
        // first choice at every size: the kernel reads the items from, and writes the answers to, pinned host memory itself -- one launch, one
        // synchronisation, no copy engine, no turn-taking between callers
        int rc = check_pass_local_host(h, c, items, (uint32_t)n, perm_out, err_out, &tried);
        if (tried) walk_outcome(h, c, n, rc);
        if (rc != kTakeLevelLoop) return rc;
        // a block ran out of private frontier (-> the level loop below), or the batch needs more units than blocks (-> the copying walk below)
    }
    if (!items_on_device) HIP_TRY(c->d_items.ensure(n));  // (a grow-only buffer whose contents an ensure() may discard)
    HIP_TRY(c->d_perm.ensure(n));
    HIP_TRY(c->d_errout.ensure(n));
    if (!items_on_device) {
        const void *src = items;
        if ((const void *)items != c->h_in.p && !h->is_pinned(items, n * sizeof(acl_item_t))) {  // (the string entry points intern straight into the staging buffer)
            HIP_TRY(c->h_in.ensure(n * sizeof(acl_item_t)));
            std::memcpy(c->h_in.p, items, n * sizeof(acl_item_t));
            src = c->h_in.p;
        }
        HIP_TRY(hipMemcpyAsync(c->d_items.p, src, n * sizeof(acl_item_t), hipMemcpyHostToDevice, c->stream));
    }
    const bool pin_p = h->is_pinned(perm_out, n), pin_e = !err_out || h->is_pinned(err_out, n * sizeof(int32_t));
    uint8_t *hp = perm_out;
    int32_t *he = err_out;
    if (!pin_p || !pin_e) {
        HIP_TRY(c->h_out.ensure(n * 5 + 64));
        if (!pin_e) he = (int32_t *)c->h_out.p;
        if (!pin_p) hp = (uint8_t *)c->h_out.p + n * 4;
    }
    auto results_d2h = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(hp, c->d_perm.p, n, hipMemcpyDeviceToHost, c->stream));
        if (err_out) HIP_TRY(hipMemcpyAsync(he, c->d_errout.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        return ACL_OK;
    };
    // (What is left of the copying path: batches the host-mapped walk above does not take -- switched off, backing off after an overflow, beyond
    // its sub-pass limit.)  ONE launch where the single-launch walk takes it: H2D, kernel, overflow-flag read-back and result copies all go onto
    // the stream and the host synchronises ONCE.  Only a walk that overflowed its private regions comes back for the level loop.
    int rc = kTakeLevelLoop;
    if (allowed && !tried) {
        tried = true;
        HIP_TRY(c->d_has.ensure(std::max<size_t>(n, 4096)));
        HIP_TRY(c->d_err.ensure(std::max<size_t>(n, 4096)));
        // chip-filling batches of several callers: kernels one at a time (host mutex, held from the launch to the one synchronisation); the
        // next caller's H2D, already enqueued on its own stream, runs meanwhile
        std::unique_lock<std::mutex> tk(c->dev->compute_mu, std::defer_lock);
        if (n >= kComputeTokenItems) tk.lock();
        rc = local_enqueue(h, c, h->dev_graph(c), c->d_items.p, (uint32_t)n, c->d_perm.p, c->d_errout.p);
        if (!rc) {
            rc = results_d2h();
            if (rc) return rc;
            rc = local_finish(h, c, (uint32_t)n);
        } else if (rc != kTakeLevelLoop) {
            (void)hipStreamSynchronize(c->stream);
        }
        walk_outcome(h, c, n, rc);
    }
    if (rc == kTakeLevelLoop) {  // a block ran out of private frontier, or the walk is switched off / backing off: the level loop, one batch at a time
        HIP_TRY(hipStreamSynchronize(c->stream));
        {
            std::unique_lock<std::mutex> tk(c->dev->compute_mu, std::defer_lock);
            if (n >= kComputeTokenItems) tk.lock();
            rc = check_device(h, c, c->d_items.p, n, c->d_perm.p, c->d_errout.p, !tried);  // (ends with the context's stream synchronised; a batch the walk has not tried -- sub-batched ones -- tries it per pass)
        }
        if (rc) return rc;
        rc = results_d2h();
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
        ev_collect(c);
    }
    if (rc) return rc;
    if (!pin_p) std::memcpy(perm_out, hp, n);
    if (err_out && !pin_e) std::memcpy(err_out, he, n * sizeof(int32_t));
    return ACL_OK;
}

}  // namespace aclint

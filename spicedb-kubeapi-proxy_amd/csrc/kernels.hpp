// kernels.hpp -- launch interface of the gfx950 frontier-expansion kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "plan.hpp"

namespace acl {

// frontier geometry
constexpr uint32_t kChunk = 1024;         // entries per frontier chunk (16 KiB)
constexpr uint32_t kSegsPerChunk = kChunk / 64;
constexpr uint32_t kMaxFrontierChunks = (1u << 18) - 1;  // 16 B entries of a frontier buffer stay below 4 GiB: the kernels address with 32-bit byte offsets
constexpr uint32_t kMaxLevels = 50;       // dispatch max depth, reference pkg/spicedb/spicedb.go:34
constexpr uint32_t kLevelSlots = 128;     // per-iteration counters (the sharded reverse walk runs two iterations per level)
constexpr uint32_t kMaxShards = 64;      // per-destination export counters (all-to-all exchange)
constexpr uint32_t kStatusWords = 2 * kLevelSlots + 2 + kMaxShards;  // nchunks[] | any[] | overflow | export count | export count per destination
constexpr uint32_t kDeadMeta = 0xFFFFFFFFu;
constexpr int kWavesPerBlock = 4;
constexpr uint32_t kProgLdsEntries = 256;  // ops + progs (32 B each) cached in LDS when they fit

// per-item status byte written by the kernels
enum : uint8_t { ITEM_ERR_NONE = 0, ITEM_ERR_DEPTH = 1, ITEM_ERR_INVALID = 2 };

// frontier entry: one pending sub-check (req, state) -- 16 B, one dwordx4 per lane
//   x = object id, y = request index, z = meta, w = subject id of the request
//   meta = slot[0:13) | level[13:19) | probed[19] | subject key[20:32)
struct DevGraph {
    const uint32_t *meta, *edges, *buckets;  // plan.hpp: row descriptors (uint2), sorted rows, hashed 4-slot buckets (uint4)
    const FwdOp *ops;
    const SlotProg *progs;
    const uint32_t *type_slot_base, *type_nmembers;
    uint32_t nslots, ntypes, nops;
    // combine programs (schemas with `&` / `-`, plan.hpp SlotProg::combine); all unused by the monotone instantiations
    const uint32_t *bexpr = nullptr;   // boolean programs
    uint4 *nodes = nullptr;            // CombineNode records the walk appends (single launch: node_cap per block; level loop: node_cap in all)
    uint32_t *ccount = nullptr;        // level loop: {leaf cells handed out, nodes appended} (the single-launch walk counts in LDS)
    uint32_t node_cap = 0, cell_cap = 0;  // per block (single launch) / in all (level loop)
    uint32_t cell0 = 0;                // index of the first leaf cell in has[] / err[] (= the batch size: cells follow the requests' own)
    uint32_t walk_flags = 0;           // kWalkNoDirect: the single-launch walk builds every task list the general way (set by the host after a walk met a
                                       // pair of segments with more children than the direct form's head-bit window: kernels.hip, process_segment)
    // the snapshot's hot hashed class (Snapshot::hot_*, plan.cpp choose_hot_class): the single-launch walk keeps every request's row descriptor of this class
    // in LDS for the length of a unit (kernels.hip, k_check_local's s_sd).  hot_cnrows == 0: none
    uint32_t hot_cbase = 0, hot_cnrows = 0, hot_ckey = 0;
    // the snapshot's two-hop rows (Snapshot::hop2_*): one {start, end} descriptor per object of hop2_slot's type at meta[hop2_base + id]; the direct form of the
    // single-launch walk expands states of that slot from them.  hop2_nrows == 0: none (never built, or dropped by a patch)
    uint32_t hop2_base = 0, hop2_nrows = 0, hop2_slot = 0xFFFFFFFFu;  // hop2_slot: no slot's number while the rows are not in use (none, dropped, or kWalkNoHop2)
};
constexpr uint32_t kWalkNoDirect = 1u;
constexpr uint32_t kWalkNoHop2 = 2u;  // ACL_HOP2=0 (A/B and tests, one library for both forms): the walk reads the one-hop rows even where two-hop rows exist -- the host
                                      // sets the bit and, with it, hop2_slot to no slot's number: the kernel's one test per pair is the slot compare
constexpr uint32_t kOverflowPools = 8u;   // level loop on the SHARDED graph, schemas with `&` / `-`: a shard ran out of combine nodes / leaf cells -- the native loop grows the pools and redoes the batch
constexpr uint32_t kOverflowExport = 16u;  // a level's control record on the SHARDED graph (fold_headers): a shard's export block is outgrown -- apart from bit 1, a frontier out of chunks, which the
                                           // native Check loop answers by merging duplicates
constexpr uint32_t kOverflowDirect = 4u;  // single-launch walk's overflow code: "redo, and stop using the direct task lists on this snapshot"
struct DevReverse {
    const uint32_t *rmeta, *redges;  // uint2 {start, end} per (relation, class, subject); resource ids
    const RevOp *rops;
    const RevProg *rprogs, *rseeds;
    const uint64_t *rdest;          // [nslots] other shards holding parent rows of the slot's states (all-to-all form of the sharded walk)
    const uint32_t *slot_bit_base;  // [nslots]
    const uint32_t *slot_nobjects;  // [nslots] id space of the slot's type
    uint32_t *visited;              // [nreq][visited_words]
    uint32_t visited_words;
    uint32_t nslots = 0, nrops = 0;  // sizes of rprogs / rops (the single-launch walk stages them in LDS when they fit)
    // level loop (k_rev_expand) on an unsharded graph: the slots that can lead to the lookup's result slot (Snapshot::rev_useful; bit of slot x < 256) -- ops into any
    // other slot are skipped.  All ones: everything (sharded graphs: a shard's programs are not the whole slot graph).
    uint32_t useful[8] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
};
constexpr uint32_t kRevLdsRowBytes = 128u << 10;  // the result slot's rows live in LDS up to this size (1 M objects)
constexpr uint32_t kRevLdsSlots = 256, kRevLdsOps = 384;  // what k_rev_local's LDS copy of the reverse programs holds
// Chunk ids: [0, nwaves) are the waves' static first chunks (no allocation), ids >= nwaves come from the
// level's dynamic counter nchunks[iter].  counts[] holds every readable chunk's fill.
struct DevFrontier {
    uint4 *buf[2];
    uint32_t *counts[2];   // per-chunk fill
    uint32_t *nchunks;     // [kLevelSlots] dynamic chunks produced by iteration i (0 = seed)
    uint32_t *any;         // [kLevelSlots] iteration i produced at least one entry
    uint32_t *overflow;    // set when a frontier buffer ran out of chunks
    uint32_t max_chunks;
    uint32_t nwaves;       // waves of every expand launch == number of static chunks
};

// Sharded graph: pending sub-checks whose rows live on another shard leave through `exp`
// (16 B frontier entries, one contiguous buffer per level) and are exchanged by the host between levels.
// `exp_count` keeps counting past `cap` (entries beyond it are dropped) so the host can size a retry.
struct DevShard {
    uint4 *exp = nullptr;
    uint32_t *exp_count = nullptr;   // [1] all-gather form; followed by [kMaxShards] per-destination counters (all-to-all form)
    uint32_t by_dest = 0;            // != 0: `exp` is `world` buffers of `cap` entries, entry -> the buffer of the shard that owns its slot
    uint32_t cap = 0;
    uint32_t rank = 0;
    uint32_t world = 1;
    uint32_t stride = 0;             // by_dest: entries between two destinations' buffers (0 = cap: the buffers are contiguous)
};
// reverse-walk entry flags (meta = slot[0:13) | dist[13:19) | flags)
constexpr uint32_t kRevForeign = 1u << 19;  // state visited on its owner shard: expand it here, do not touch `visited`
constexpr uint32_t kRevVisited = 1u << 20;  // state already passed the visit phase
enum RevPhase : uint32_t { REV_FUSED = 0, REV_VISIT = 1, REV_EXPAND = 2 };

void launch_seed(hipStream_t s, const DevGraph &g, const DevFrontier &f, const uint4 *items, uint32_t n, uint8_t *has, uint8_t *err,
                 const DevShard &sh = DevShard());
void launch_expand(hipStream_t s, const DevGraph &g, const DevFrontier &f, uint32_t iter, uint8_t *has, uint8_t *err,
                   const DevShard &sh = DevShard());
// appends the entries of `in` (an all-gathered export buffer) whose slot this shard owns to the frontier that
// iteration `iter` produced
void launch_import(hipStream_t s, const DevGraph &g, const DevFrontier &f, uint32_t iter, const uint4 *in, uint32_t n, const DevShard &sh);
// native sharded loop: exchange-block headers written on the device (nblocks = 1: all-gather form, exp_count[0]; = world: one per destination,
// exp_count[1 + d]); import of the exchanged blocks + the level's control record {total exported, any produced, overflow code, largest block}.
// hdrs: `world` headers (one per source), data: `world` blocks of `cap` entries; have_data false: the entries were not exchanged this level
void launch_xhdr(hipStream_t s, uint4 *hdr, uint32_t nblocks, const uint32_t *exp_count, const uint32_t *any_iter, const uint32_t *overflow);
void launch_import_gathered(hipStream_t s, const DevGraph &g, const DevFrontier &f, uint32_t iter, const uint4 *hdrs, const uint4 *data, uint32_t world, uint32_t rank,
                            uint32_t cap, bool have_data, uint32_t *ctrl);
void launch_rev_import_gathered(hipStream_t s, const DevReverse &r, const DevFrontier &f, uint32_t iter, const uint4 *hdrs, const uint4 *data, uint32_t world, uint32_t rank,
                                uint32_t cap, bool have_data, uint32_t *ctrl);
void launch_rev_import(hipStream_t s, const DevReverse &r, const DevFrontier &f, uint32_t iter, const uint4 *in, uint32_t n);
void launch_rev_seed(hipStream_t s, const DevFrontier &f, const uint32_t *d_sids, uint32_t n, uint32_t key);
void launch_keep(hipStream_t s, uint32_t k_items, const uint32_t *item_off, const uint8_t *perm, uint8_t *keep_out);
// single-launch Check: units of rpw (<= 256) consecutive requests; block b (of nblocks) walks units b, b + nblocks, ... through every
// level with a private frontier of `cap` entries in each of buf0 / buf1 (regions b * cap); next_unit: zeroed device counter, needed when there are more units than blocks; *overflow != 0 afterwards: redo on the level loop
void launch_check_local(hipStream_t s, const DevGraph &g, const uint4 *items, uint32_t n, uint32_t rpw, uint32_t nblocks, uint32_t *next_unit, uint4 *buf0,
                        uint4 *buf1, uint32_t cap, uint32_t *overflow, uint8_t *has, uint8_t *err, uint8_t *perm_out, int32_t *err_out,
                        uint32_t *max_level = nullptr /* device word (zeroed): atomicMax of the dispatch levels the units needed */,
                        bool wide = false /* 12 waves per block (and unit) instead of 4: chip-filling batches */,
                        uint32_t skew = 0 /* unit u holds rpw + skew ... rpw - skew requests, falling with u (items read across PCIe arrive in block order) */,
                        uint32_t *done_ctr = nullptr /* device word, zero between launches */, uint32_t *done_flag = nullptr /* pinned host word (device pointer): the last block to
                        finish stores done_val there, behind a system-scope release of every block's answers -- the host spins on it instead of synchronising the stream */,
                        uint32_t done_val = 0, const uint4 *inline_items_host = nullptr /* HOST pointer to the batch's items: a batch of <= 4 rides in the kernel's arguments
                        and `items` is not read */);
// blocks of the single-launch kernel that are resident at once on this device
int local_grid_blocks(int device, size_t prog_bytes, bool wide = false);  // prog_bytes: (slots + ops) * 32, the kernel's dynamic LDS; wide: the wide (12-wave) instantiation
uint32_t local_unit_max(bool wide = false);  // requests per unit, at most (= threads per block of the single-launch kernel: thread i seeds request i of the unit)
// strikes duplicate (request, state, level) entries of the frontier iteration `iter` produced; table: 2^bits u64 (reset here)
void launch_dedup(hipStream_t s, const DevFrontier &f, uint32_t iter, uint64_t *table, uint32_t bits, bool cells = false);  // cells: the entries carry result cells (combine schemas): `table` is 1.5 x 2^bits words
constexpr uint32_t kDedupBatch = 1u << 14;  // requests per dedup pass (the key holds 14 request bits)
void launch_finalize(hipStream_t s, uint32_t n, const uint8_t *has, const uint8_t *err, uint8_t *perm_out, int32_t *err_out);
// level loop, schemas with `&` / `-`: evaluates the combine nodes of frontier iteration `iter` (call for iter = last .. 1: a node only depends
// on nodes of later iterations); the node count is read from g.ccount[1] on the device
void launch_resolve(hipStream_t s, const DevGraph &g, uint32_t iter, uint8_t *has, uint8_t *err);
// sharded graph, schemas with `&` / `-`: {nodes appended, cells handed out} of this shard as a 16-byte header; the gathered node lists (world blocks of `stride`
// nodes, hdrs[b].x valid ones in block b) resolved for frontier iteration `iter` (members first), on every shard alike
void launch_node_hdr(hipStream_t s, uint4 *hdr, const uint32_t *ccount);
void launch_resolve_gathered(hipStream_t s, const DevGraph &g, const uint4 *nodes, uint32_t stride, const uint4 *hdrs, uint32_t world, uint32_t iter, uint8_t *has, uint8_t *err);
void launch_rev_expand(hipStream_t s, const DevReverse &r, const DevFrontier &f, uint32_t iter, uint32_t phase = REV_FUSED,
                       const DevShard &sh = DevShard());
// single-launch LookupResources: block b walks lookup b (subject sids[b] of class `key`) through every reverse level; visited rows r.visited
// (all zero before and after), a private log of `cap` 8-byte entries per block in `logs`; the result slot's first `copy_words`
// words go to out_bitmaps + b * out_stride (device or pinned host memory; the rest of the row is zeroed), the id counts to out_counts.
// *status != 0 afterwards (the caller zeroes it; it may live in pinned host memory): redo on the level loop (1) / a row beyond the enumeration limit (2);
// out_counts[b] = ids in the row | reverse levels walked << 56
// Result rows beyond the block's LDS (a type of more than 1 M objects) of a result slot that nothing expands further (the usual case: the permission a list is
// filtered by): with `big` given the ids are marked as BYTES of a per-lookup byte map, the walk defers the heavy rows of the result slot to a chip-wide launch
// and a third launch folds the bytes into the callers' rows from all CUs (kernels.hip RevDefer) -- three launches on `s`, the completion word raised by the last.
struct RevBigRows {
    uint8_t *bytemap = nullptr;     // [n][bytemap_stride], all zero (the third launch zeroes what it found set); bytemap_stride: a multiple of 128 >= the slot's id space
    uint32_t bytemap_stride = 0;
    void *tasks = nullptr;          // [n][task_cap] x 8 bytes
    uint32_t *task_count = nullptr; // [n]
    uint32_t *levels = nullptr;     // [n]
    uint64_t *counts = nullptr;     // [n] device accumulators, zero between launches
    uint32_t task_cap = 0;
    uint32_t defer_min = 0;         // children of one round from which terminal rows are deferred (0 = the default, 4096)
};
constexpr uint32_t kRevUsefulWords = kRevLdsSlots / 32;
struct RevUseful {  // the slots a lookup has to walk (Snapshot::rev_useful's row of its result slot); all ones: everything
    uint32_t w[kRevUsefulWords];
};
// target_slot | kRevTargetSink: nothing above the result slot leads back into it (Snapshot::rev_sink) -- its states end the walk instead of being expanded
constexpr uint32_t kRevTargetSink = 0x80000000u;
void launch_rev_local(hipStream_t s, const DevReverse &r, const uint32_t *sids, uint32_t n, uint32_t key, uint32_t target_slot, void *logs,
                      uint32_t cap, uint32_t *out_bitmaps, uint32_t out_stride, uint32_t copy_words, uint64_t *out_counts, uint32_t *status,
                      uint32_t lds_row_words /* words covering the result slot's id space: kept in LDS when <= kRevLdsRowBytes, else (or 0) in r.visited */,
                      uint32_t *done_ctr = nullptr, uint32_t *done_flag = nullptr, uint32_t done_val = 0 /* as launch_check_local: the last block stores done_val into the pinned
                      word done_flag behind a system-scope release of every block's rows, counts and status */,
                      const RevBigRows *big = nullptr, const RevUseful *useful = nullptr /* NULL: every slot */);
// single-launch LookupResources against MANY result slots (kernels.hip k_rev_multi): block b walks lookup b once and hands back one row per target --
// targets[j].copy_words words of slot targets[j].slot's rows at out_bitmaps + b * out_stride + targets[j].out_off, zero up to out_words; out_counts[b * n_targets + j] =
// ids in that row | reverse levels walked << 56.  `targets` is read by the device (device or pinned host memory).  useful: the OR of the targets'
// Snapshot::rev_useful rows; is_target: bit of every target slot.  r.visited all zero before and after; logs, cap, status and the completion word as launch_rev_local.
struct RevMultiTarget {
    uint32_t slot, out_off, copy_words, out_words;
};
void launch_rev_multi(hipStream_t s, const DevReverse &r, const uint32_t *sids, uint32_t n, uint32_t key, const RevMultiTarget *targets, uint32_t n_targets, void *logs,
                      uint32_t cap, uint32_t *out_bitmaps, uint32_t out_stride, uint64_t *out_counts, uint32_t *status, const RevUseful &useful, const RevUseful &is_target,
                      uint32_t *done_ctr = nullptr, uint32_t *done_flag = nullptr, uint32_t done_val = 0);
// single-launch LookupSubjects (kernels.hip k_subj_local): block b walks the forward programs from resource rids[b] of `target_slot` and marks the ids of the
// subjects of `key` it reaches in rows + b * row_words (device memory; zeroed by the caller when the row does not fit the block's LDS: row_words * 4 >
// kRevLdsRowBytes); flags_out[b] = 1 when a `T:*` row was reached.  visited: [n][g.visited_words] zeroed by the caller; logs: [n][cap] 8-byte entries.
// *status != 0 afterwards (the caller zeroes it): 1 = a block's log overflowed (redo with a larger cap), 2 = a row beyond the per-task enumeration limit.
struct DevSubjects {
    const uint32_t *meta, *edges;  // the forward snapshot's sorted rows
    const FwdOp *ops;
    const SlotProg *progs;
    const SubjOp *sops;            // [nops] side table (plan.hpp)
    const uint32_t *smeta, *sids;  // subject rows
    const uint32_t *slot_vbase, *slot_vn;
    uint32_t nslots, nops, visited_words, max_ops, max_ops_rel;
};
constexpr uint32_t kSubjLdsProgBytes = 16u << 10;  // programs + ops + side table staged in LDS up to this size
void launch_subj_local(hipStream_t s, const DevSubjects &g, const uint32_t *rids, uint32_t n, uint32_t target_slot, uint32_t key, void *logs, uint32_t cap,
                       uint32_t *visited, uint32_t *rows, uint32_t row_words, uint32_t *flags_out, uint32_t *status);
// single-launch Explain (kernels.hip k_explain_local): block b walks the forward programs from item b's resource, by the walk k_subj_local uses, until the level at
// which the item's ONE subject is found, and writes the path that led there.  items: [n] {resource id, target slot, subject key, subject id}; buckets: the forward
// snapshot's hashed rows (DevGraph::buckets); logs: [n][cap] 16-byte entries; visited: [n][g.visited_words] zeroed by the caller.
//   counts[b] = records written | state << 16 (kExplainFound: a path; kExplainNotFound: no level produced a hit, or the walk stopped; kExplainBadTrace: the
//               log did not lead back to entry 0)
//   traces[b * kExplainTraceRecs ...] = {op index, parent object id, child object id, flags (kExplainRecWild: the child is the op's `T:*` id)} in path order --
//               one record per state on the path below the root (the op that produced it) and, unless the hit was a reflexive op's, one for the hit itself
// *status != 0 afterwards (the caller zeroes it): 1 = a block's log overflowed (redo with a larger cap), 2 = an enumerated row beyond kSubjMaxRow.
constexpr uint32_t kExplainTraceRecs = kMaxLevels + 1;
constexpr uint32_t kExplainFound = 0, kExplainNotFound = 1, kExplainBadTrace = 2;
constexpr uint32_t kExplainRecWild = 1u;
void launch_explain_local(hipStream_t s, const DevSubjects &g, const uint32_t *buckets, const uint4 *items, uint32_t n, void *logs, uint32_t cap, uint32_t *visited,
                          uint4 *traces, uint32_t *counts, uint32_t *status);
// single-launch Explain for revocation (kernels.hip k_revoke_local): block b walks item recs[2b] = {resource id, target slot, subject key, subject id} as
// k_explain_local does, with the stored relationship recs[2b + 1] = {class, resource id, subject id, 1 when the class is a `T:*` class} left out: no terminal
// test counts it and no enumerated row yields it.  op_class: [g.nops] the class number of the relationships each op reads (any number no mask carries for an
// op that reads none).  found_out[b] = kRevokeFound (the subject is still found), kRevokeNotFound (the closure ran dry without it) or kRevokeStopped (with
// *status raised as for launch_explain_local).  logs: [n][cap] 8-byte entries; visited: [n][g.visited_words] zeroed by the caller.
constexpr uint32_t kRevokeFound = 0, kRevokeNotFound = 1, kRevokeStopped = 2;
void launch_revoke_local(hipStream_t s, const DevSubjects &g, const uint32_t *buckets, const uint32_t *op_class, const uint4 *recs, uint32_t n, void *logs,
                         uint32_t cap, uint32_t *visited, uint32_t *found_out, uint32_t *status);
// single-launch Explain denial (kernels.hip k_reach_local): block b walks the forward programs from roots[b] = {resource id, target slot} by the same walk,
// following children only, and hands back the distinct states it reached, each at its least dispatch level: out.spans[b] = {first record, count} of
// out.recs, records {object id, slot | level << 16} in no particular order.  out.total (zeroed by the caller) counts the records of ALL blocks, also of
// those that did not fit out.cap -- they raise *out.overflow (zeroed by the caller) and copy nothing.  logs: [n][cap] 8-byte entries; visited and *status as
// for launch_subj_local.
struct DevReachOut {
    uint2 *recs;
    uint32_t cap;
    unsigned long long *total;
    uint2 *spans;  // [n]
    uint32_t *overflow;
};
void launch_reach_local(hipStream_t s, const DevSubjects &g, const uint2 *roots, uint32_t n, void *logs, uint32_t cap, uint32_t *visited, const DevReachOut &out,
                        uint32_t *status);
// level-synchronous LookupSubjects (kernels.hip k_subj_expand; the sharded graph's native loop): one launch per dispatch level over the chunked frontier, all
// lookups of a chunk at once.  visited: [m][g.visited_words], rows: this shard's PARTIAL rows [m][row_words], flags: [m] bytes (1: a `T:*` row was reached) --
// all zeroed by the caller.  A row beyond the per-task enumeration limit raises overflow code 2 in the frontier's status block.
struct DevSubjLevel {
    DevSubjects g;
    uint32_t *visited;
    uint32_t *rows;
    uint8_t *flags;
    uint32_t row_words;
    uint32_t key;  // the subjects' class
};
// seeds (lookup i starts from rids[i] of target_slot, on the shard that owns the slot's type) + the status block
void launch_subj_seed(hipStream_t s, const DevSubjLevel &g, const DevFrontier &f, const uint32_t *rids, uint32_t n, uint32_t target_slot, const DevShard &sh);
void launch_subj_expand(hipStream_t s, const DevSubjLevel &g, const DevFrontier &f, uint32_t iter, const DevShard &sh);
// as launch_import_gathered: keeps the exchanged entries whose slot this shard owns (deciding the visits of the ones due next) + the level's control record
void launch_subj_import_gathered(hipStream_t s, const DevSubjLevel &g, const DevFrontier &f, uint32_t iter, const uint4 *hdrs, const uint4 *data, uint32_t world,
                                 uint32_t rank, uint32_t cap, bool have_data, uint32_t *ctrl);
// out[m][out_stride] = OR over the `world` gathered partial rows [world][m][row_words] (words behind row_words: zero)
void launch_subj_fold(hipStream_t s, const uint32_t *gathered, uint32_t world, uint32_t m, uint32_t row_words, uint32_t *out, uint32_t out_stride);
// Watch sets (engine_watchset.cpp): the records of new XOR old over n_rows rows, ordered by (row, bit) -- three launches on `s`.  Rows are packed
// ([row][words], 16-byte aligned bases); the old rows may be narrower or wider than the new ones and there may be fewer of them (old_nrows): whatever
// is not there reads as zero, and neither array is read past its end.  A tile is kDiffTileWords words of one row, walked by one wave in steps of
// 64 lanes x 4 words (one 16-byte load per lane and array where both widths are multiples of 4, word loads otherwise).
//   count: tile_counts[row * ntiles + tile] = popcount(old ^ new) over the tile
//   scan : offs[i] = sum of tile_counts[0 .. i) as 64-bit, offs[n_rows * ntiles] = the total
//   emit : record k of a tile at out[offs[tile] + k] = {row_ids ? row_ids[row] : row, bit, bit of NEW (1 gained, 0 lost), 0}, one 16-byte store each;
//          nothing is written at or beyond out_cap
// row_ids[row] == kDiffSkipRow: the row contributes nothing (a watcher whose baseline is "now").
constexpr uint32_t kDiffTileWords = 4096;
constexpr uint32_t kDiffSkipRow = 0xFFFFFFFFu;
struct DevRowsDiff {
    const uint32_t *old_rows, *new_rows;
    uint32_t old_words, new_words;  // words per row
    uint32_t old_nrows, n_rows;
    const uint32_t *row_ids;        // [n_rows] or NULL
};
inline uint32_t rows_diff_tiles(const DevRowsDiff &d) { return (std::max(d.old_words, d.new_words) + kDiffTileWords - 1) / kDiffTileWords; }  // per row
void launch_rows_diff_count(hipStream_t s, const DevRowsDiff &d, uint32_t *tile_counts, uint64_t *offs);  // count + scan
void launch_rows_diff_emit(hipStream_t s, const DevRowsDiff &d, const uint64_t *offs, uint4 *out, uint64_t out_cap);
// Lookup cursors (engine_cursor.cpp): pages of ids out of packed rows ([n_rows][row_words], row_words a multiple of 4) and their rank index -- offs as
// launch_rows_diff_count leaves it for these rows against an empty old array ([n_rows * ntiles + 1], ntiles = tiles of kDiffTileWords words per row).
// Request q = {row, after_id, limit, base}: the ascending ids of the row that are > after_id (0xFFFFFFFF: from id 0), at most `limit` of them, at
// ids[base ..]; res[q] = how many | 0x80000000 when a larger id remains.  row < n_rows and base + limit inside `ids` are the caller's to check.
// Two launches on `s` (a plan step of one wave per request into plan[m] of 16 bytes each, then one wave per (request, tile)); nothing is synchronised.
struct DevRowsPage {
    const uint32_t *rows;
    const uint64_t *offs;
    uint32_t row_words, ntiles, n_rows;
};
void launch_rows_page(hipStream_t s, const DevRowsPage &p, const uint4 *reqs, uint32_t m, void *plan, uint32_t *res, uint32_t *ids);
// Derived lookup cursors (engine_cursor.cpp): n_exprs new rows of out_words words (a multiple of 4), each a boolean combination of rows that already live on
// this device.  Expression e = exprs[e] = {first, n_any, n_all, n_none} owns the operand records ops[first ..): its any-list, then its all-list, then its
// none-list; its row is (OR of the any-list, or everything when n_any == 0) AND (every row of the all-list) AND NOT (OR of the none-list), n_any + n_all >= 1.
// An operand record is 16 bytes, {device address of the row (16-byte aligned), words of the row (a multiple of 4, at most out_words) in the low half of the
// second 8 bytes}: words an operand does not have read as zero and no operand is read past its end.  Bits behind the type's last id must be zero in every
// operand; they are zero in the result.  out == NULL: count mode, no row is written.  Two launches on `s`, whatever n_exprs and the lists' lengths are: one
// wave per (expression, tile of kDiffTileWords words) leaves the tile's popcount in tile_counts[e * ntiles + tile], then the diff's scan turns the counts into
// the rank index offs[n_exprs * ntiles + 1] that launch_rows_page reads.  Nothing is synchronised; n_exprs == 0: nothing is launched.
struct DevRowsDerive {
    const void *exprs;  // [n_exprs] 16-byte expression records
    const void *ops;    // 16-byte operand records
    uint32_t *out;      // [n_exprs][out_words] or NULL
    uint32_t out_words, ntiles, n_exprs;
};
void launch_rows_derive(hipStream_t s, const DevRowsDerive &d, uint32_t *tile_counts, uint64_t *offs);
// Subject-direction watch sets (engine_watchset.cpp subject_rows): the candidates of a permission with `&` / `-` / `.all()` confirmed on the device.  One slice of
// whole rows [row0, row0 + rows of the slice) of a packed row array at a time:
//   fill  : rows wrows[0 .. nflag) (the walk reached `T:*` there) become "every id of the type": bits [0, nobj) set, the wildcard's own bit cleared
//   items : record k of the slice's diff against an empty old array ({row of the slice, bit, 1, 0}: k_rows_diff_emit without row ids) -> the 16-byte item
//           {head, rids[row0 + row], tail, bit}; behind the nrec records one stand-in per flagged row of the slice, wrows[wrow0 .. wrow0 + nstand), whose
//           subject is fresh_sid (an id nobody names: the wildcard as a Check sees it)
//   apply : answer k of a Check over those items: not `has_value`, or an error -> the record's bit is cleared (lanes that share a word fold first, one
//           agent-scope atomic AND per word and wave); a stand-in's answer becomes its row's flag word; the least index of an erring item is left in
//           *status by atomic minimum (the caller stores 0xFFFFFFFF first)
//   wild  : rows whose flag word is set get the wildcard's bit
struct DevRefine {
    uint32_t *rows;          // [n_rows][row_words]
    uint32_t *flags;         // [n_rows]
    const uint32_t *rids;    // [n_rows] the rows' resources
    const uint32_t *wrows;   // ascending indices of the rows the walk flagged
    const uint4 *recs;       // the slice's candidate records
    uint32_t row_words, row0, nrec, wrow0, nstand;
    uint32_t head, tail;     // an item's first and third word: resource type | permission << 16, subject type | subject relation << 16
    uint32_t fresh_sid;
};
// the walk's packed rows (k_subj_local: [m][src_words]) into rows of dst_words >= src_words words, the words behind src_words zeroed, and their flag words
void launch_subj_rows_store(hipStream_t s, const uint32_t *src, uint32_t src_words, const uint32_t *src_flags, uint32_t m, uint32_t *dst, uint32_t dst_words, uint32_t *dst_flags);
void launch_refine_fill(hipStream_t s, const DevRefine &r, uint32_t nflag, uint32_t need /* words that hold the type's ids */, uint32_t nobj, uint32_t wid);
void launch_refine_items(hipStream_t s, const DevRefine &r, uint4 *items);
void launch_refine_apply(hipStream_t s, const DevRefine &r, const uint8_t *perm, const int32_t *err, uint32_t has_value, uint32_t *status);
void launch_refine_wild(hipStream_t s, uint32_t *rows, uint32_t row_words, const uint32_t *flags, uint32_t n_rows, uint32_t wid);
// Explain proofs (engine_proof.cpp): one round of the search asks, for each of `ngroups` goals, about a run of candidate objects -- the members of a row the
// goal may step to -- that share the goal's {resource type | permission << 16, subject type | relation << 16, subject id}.  Candidates of a group are
// neighbours, group g's start at groups[g].w.
//   items : candidate k -> the 16-byte item {head, obj[k], tail, subject} of its group, one store per lane
//   pick  : the answers of a Check over those items, folded per group where they are: first[2 g] / first[2 g + 1] = the least index INSIDE the group of a
//           candidate that answered HAS / NO without error (the caller stores 0xFFFFFFFF first), count[2 g] / count[2 g + 1] = how many did (the caller
//           stores 0 first).  A wave whose lanes share one group folds by ballot and issues one set of agent-scope atomics; 16 bytes per group reach the host
struct DevProofPick {
    const uint32_t *obj;    // [ncand] candidate object ids
    const uint32_t *group;  // [ncand] the candidate's group
    const uint4 *groups;    // [ngroups] {head, tail, subject id, index of the group's first candidate}
    uint32_t ncand, ngroups;
    uint32_t *first, *count;  // [2 ngroups] each
};
//   winner: win[2 g] / win[2 g + 1] = the object ids of those two candidates (0xFFFFFFFF: none), so a row the device enumerated never has to reach the host
//   rows  : groups whose candidates are a whole sorted sub-row of the forward graph from its `floor`-th id on (rows[g] = {descriptor index, floor}; a
//           descriptor index >= meta_pairs: not such a group, left alone) are enumerated where the row is -- one block per group reserves the row's length
//           in the candidate region by one agent-scope add to total[0 .. 1] (64 bits, the caller stores the host-made candidates' count), writes its
//           start into groups[g].w and its length into gn[g], and copies the ids; a row that does not fit into `cap` raises total[2] and copies nothing
struct DevProofRows {
    const uint32_t *meta, *edges;  // DevGraph's
    uint32_t meta_pairs, nedges;   // their valid lengths (uint2 descriptors, ids)
    const uint2 *rows;             // [ngroups]
    uint4 *groups;                 // [ngroups]
    uint32_t *gn;                  // [ngroups]
    uint32_t *obj, *group;         // [cap]
    uint32_t cap, ngroups;
    uint32_t *total;               // [3]
};
void launch_proof_rows(hipStream_t s, const DevProofRows &r);
void launch_proof_winner(hipStream_t s, const DevProofPick &p, uint32_t *win);
void launch_proof_items(hipStream_t s, const DevProofPick &p, uint4 *items);
void launch_proof_pick(hipStream_t s, const DevProofPick &p, const uint8_t *perm, const int32_t *err, uint32_t has_value, uint32_t no_value);
// blocks per expand launch for this device (all co-resident); nwaves = blocks * kWavesPerBlock
int expand_grid_blocks(int device);

}  // namespace acl

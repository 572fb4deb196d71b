// kernels.hip -- gfx950 (CDNA4) frontier-expansion kernels of the batched ACL-check engine.
//
// What they replace: the per-item recursive dispatch SpiceDB runs for CheckBulkPermissions (reached from reference
// pkg/authz/check.go:48 and pkg/authz/postfilter.go:134) and the reverse walk behind LookupResources (pkg/authz/lookups.go:65).
// A pending sub-check is a 16-byte frontier entry (object id, request, slot | level | flags, subject id); a SEGMENT is 64 of them,
// one per lane.  process_segment() advances a segment by one dispatch level:
//   - every lane interprets its state's flattened program (plan.hpp, cached in LDS): probes of the request's subject in hashed rows
//     (4-slot buckets, seeded single-choice: ONE 16 B gather per test -- two-choice rows, two gathers, only where no seed was found;
//     never a probing chain) or sorted rows (binary search), and "enumerate" operations whose child states are produced by a wave-cooperative, load-balanced expansion:
//       - per-lane tasks (row start, degree, the subject's hashed row) are compacted into LDS with wave64 ballot + mbcnt,
//       - a DPP prefix sum over task degrees sizes the work, and every task marks its first work item with a head bit,
//       - lanes take consecutive work items, find their task from the head bits (two v_mbcnt) and load consecutive edges of a row,
//       - each child's own probes are evaluated RIGHT THERE; only children that still have something to enumerate are written,
//         compacted with a second ballot, as consecutive entries.  Leaf states never enter the frontier.
//   - where a segment is uniform enough the interpreter is bypassed: already-probed single-op parents (the deep levels) fetch has[],
//     their row descriptor and the subject's row of the child's probe in ONE trip, two segments at a time; segments of ONE slot build
//     their task list with the prefix sums taken in registers (the direct form, round 5); simple_steps expands the tasks kSimpleWidth
//     children per lane and step; flush_probes handles arrow-target states.
//   Loads are pinned into trips (issue_fence): all loads of a trip are issued before the first of them is waited for.
//   What a wave pays for is the vector-memory INSTRUCTION, not the lane or the byte (profiles/vmem_per_pair_ab.txt): the subject's row descriptor of the hot hashed
//   class is fetched once per request (LDS), and an expansion's last step is only as wide as its children.
// Two drivers call it:
//   k_check_local  ONE launch per batch: a block walks its share of the requests through every level inside a block-private
//                  frontier region (LDS cursors, one barrier per level).  The default for every batch size.
//   k_expand       one launch per level over a chunked global frontier (every wave owns one static 16 KiB chunk per level, further
//                  chunks from one atomicAdd per 1024 entries): the sharded graph, and batches that outgrow the private regions.
// The reverse walk (LookupResources): k_rev_local, one block per lookup through every reverse level (result rows in LDS for types up to 1 M objects;
// beyond that k_rev_terminal marks the deferred heavy rows chip-wide and k_rev_rows folds the byte marks into the caller's rows); k_rev_expand is its
// level-loop form (sharded graph, overflows).  k_dedup merges duplicate entries of a level when a frontier explodes.
//
// Bound (profiles/r06_pmc_c4.md, r06_ab_check_local.txt): the CHAIN of dependent trips a wave makes per pair of segments, not HBM and
// (round 6's A/Bs) not instruction issue -- no MFMA anywhere by design.
#include <algorithm>
#include <type_traits>

#include "kernels.hpp"

namespace acl {
namespace {

constexpr int kBlock = kWavesPerBlock * 64;
#ifndef ACL_MIN_WAVES_PER_SIMD
#define ACL_MIN_WAVES_PER_SIMD 6  // (k_expand, k_rev_expand; the single-launch kernel has its own bound below)
#endif
constexpr uint32_t kTaskCap = 128;  // LDS task slots per wave
constexpr uint32_t kHeadWords = 32;  // flush_simple maps work items to tasks through head bits: rounds of <= 64 * kHeadWords children
constexpr uint32_t kSelfBit = 0x80000000u;      // task: the child is the same object (start holds its id)
constexpr uint32_t kLeafAuthBit = 0x40000000u;  // task: the row's edges carry authoritative leaf flags
constexpr uint32_t kAllBit = 0x20000000u;       // task (combine schemas): the tupleset of an intersection arrow -- every child gets a result cell of its own (OP_ALL)
constexpr uint32_t kCountMask = 0x1FFFFFFFu;
constexpr uint32_t kMaxRow = 1u << 25;  // rows longer than this cannot be enumerated in one task
constexpr uint32_t kNoSpace = 0xFFFFFFFFu;

// entry meta: slot[0:13) | level[13:19) | probed[19] | subject key[20:32)
constexpr uint32_t kProbedBit = 1u << 19;
__device__ __forceinline__ uint32_t meta_slot(uint32_t m) { return m & 0x1FFFu; }
__device__ __forceinline__ uint32_t meta_level(uint32_t m) { return (m >> 13) & 63u; }
__device__ __forceinline__ uint32_t meta_key(uint32_t m) { return m >> 20; }
__device__ __forceinline__ uint32_t make_meta(uint32_t slot, uint32_t level, uint32_t key) { return slot | (level << 13) | (key << 20); }

__device__ __forceinline__ uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
__device__ __forceinline__ uint32_t lanes_below(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
__device__ __forceinline__ uint32_t uniform(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
// Everything above this line is issued before anything below it.  Placed between "issue every load of this trip" and "first use":
// left alone, the compiler sinks a load next to its use and waits for it before it issues the next one -- a wave's independent
// gathers then travel one after the other instead of together (seen in the ISA of every multi-load step of this file).
__device__ __forceinline__ void issue_fence() { __builtin_amdgcn_sched_barrier(0); }
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// Wave64 scan / reduction on the DPP lane network: six v_add / v_max with a DPP source operand, no LDS traffic (ds_bpermute)
// and -- what mattered more here -- no per-distance lane-address VGPRs that the compiler hoists and keeps alive across the
// whole kernel.  row_shr:n shifts within a row of 16 lanes (lanes without a source add 0), row_bcast:15 / :31 carry a
// row's / a half's total into the rows above (gfx9 family incl. gfx950).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_or0(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);
}
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, uint32_t) {
    v += dpp_or0<0x111, 0xf>(v);  // row_shr:1
    v += dpp_or0<0x112, 0xf>(v);  // row_shr:2
    v += dpp_or0<0x114, 0xf>(v);  // row_shr:4
    v += dpp_or0<0x118, 0xf>(v);  // row_shr:8  -> inclusive within each row of 16
    v += dpp_or0<0x142, 0xa>(v);  // row_bcast:15 into rows 1 and 3
    v += dpp_or0<0x143, 0xc>(v);  // row_bcast:31 into rows 2 and 3
    return v;
}
__device__ __forceinline__ uint32_t wave_last(uint32_t v) { return (uint32_t)__builtin_amdgcn_readlane((int)v, 63); }
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {  // same network with max (0 is neutral for unsigned); lane 63 ends up with the maximum
    v = max(v, dpp_or0<0x111, 0xf>(v));
    v = max(v, dpp_or0<0x112, 0xf>(v));
    v = max(v, dpp_or0<0x114, 0xf>(v));
    v = max(v, dpp_or0<0x118, 0xf>(v));
    v = max(v, dpp_or0<0x142, 0xa>(v));
    v = max(v, dpp_or0<0x143, 0xc>(v));
    return wave_last(v);
}

// Phase timing (variant builds only, tools/phases.sh): every wave adds the shader-clock time between two marks to the phase named by
// the second one; loads are waited for AT the mark, so a "wait" phase is the exposed latency of that trip.  ~10 % slower.
#ifndef ACL_PROFILE_PHASES
#define ACL_PROFILE_PHASES 0
#endif
enum { PH_OTHER = 0, PH_ENTRIES, PH_GATHERS, PH_TASKS, PH_PROLOGUE, PH_EDGES, PH_BUCKETS, PH_PUSH, PH_GENERIC, PH_BARRIER, PH_SEED, PH_COUNT };
#if ACL_PROFILE_PHASES
__device__ unsigned long long acl_phase_cycles[20];
#define ACL_MARK(wo, ph)                                                                  \
    do {                                                                                  \
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                       \
        const uint32_t now_ = (uint32_t)__builtin_amdgcn_s_memtime();                     \
        if (lane_id() == 0) {                                                             \
            (wo).cold->prof[ph] += now_ - (wo).cold->last;                                \
            (wo).cold->last = now_;                                                       \
        }                                                                                 \
    } while (0)
#else
#define ACL_MARK(wo, ph) do {} while (0)
#endif

// LDS-staged task list of one wave.
// A task record is 16 bytes.  (A 20-byte record, whose 5-dword stride is coprime with the 32 banks, removes the 4-way conflicts of the per-child
// reads but was not faster and costs 6 KB of LDS per block: profiles/r06_ab_check_local.txt)
struct TaskRec {
    uint32_t x, y, z, w;
    __device__ __forceinline__ TaskRec &operator=(const uint4 &v) {
        x = v.x; y = v.y; z = v.z; w = v.w;
        return *this;
    }
    __device__ __forceinline__ operator uint4() const { return make_uint4(x, y, z, w); }
};
struct TaskLds {
    TaskRec a[kTaskCap];       // x: first edge (absolute index) -- or the object id for a "self" task; flush_simple turns it into "first edge minus
                               //    first work item" (edge index = x + work item).  y, z: the hashed row the children are probed in (first bucket,
                               //    bucket count; {0, 1} = the reserved empty bucket).  w: the request.  One 16-byte read per child instead of four.
    uint32_t count[kTaskCap];  // degree (| kSelfBit | kLeafAuthBit)
    uint32_t meta[kTaskCap];   // child meta
    uint32_t sid[kTaskCap];
    uint32_t scan[64];         // generic expansion / flush_probes: exclusive prefix of a round's 64 degrees
    uint64_t heads[kHeadWords];  // flush_simple: bit (w & 63) of word (w >> 6) set <=> a task's children start at work item w
};

// Wave-private output cursor, all fields wave-uniform.
//   chunked (k_expand, k_rev_expand): the wave starts on its static chunk (id = wave index); when that is full it closes it
//            (count store) and takes a dynamic chunk from the level's counter;
//   LOCAL   (k_check_local): a linear wave-private region [cur, cur + cap) of the frontier buffer.
struct WaveOutCold {  // what only the chunk switch / overflow paths need: kept in LDS, not in ~10 SGPRs for the whole kernel
    uint32_t *counts, *nchunks, *overflow;
    uint32_t nwaves, max_chunks, cap;
#if ACL_PROFILE_PHASES
    uint32_t last, prof[20];  // [0, PH_COUNT): phase cycles; [12, 20): counters (process_segment, simple_step; 18, 19: pairs expanded from two-hop rows / that fell back)
#endif
};
struct WaveOut {
    uint4 *buf;
    uint32_t cur, fill, produced;
    WaveOutCold *cold;  // LDS
    uint32_t *lfill;    // LOCAL: the block's output cursor (LDS) -- the block's waves append to one region
    uint32_t first;     // LOCAL: first request of the unit being walked (8-byte entries hold the request's index inside the unit)
    uint32_t lcap;      // LOCAL: entries of the block's region (a kernel constant: kept here, not behind an LDS read per reservation)
    const uint2 *ssd;   // LOCAL, 8-byte entries: the unit's requests' row descriptors of the hot hashed class (LDS, k_check_local's s_sd)
};
// room for `need` (<= kChunk) consecutive entries; returns the first entry index
template <bool LOCAL>
__device__ __forceinline__ uint32_t reserve(WaveOut &wo, uint32_t need, uint32_t lane) {
    if (wo.cur == kNoSpace) return kNoSpace;
    if (LOCAL) {
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(wo.lfill, need);
        base = uniform(base);
        if (base + need > wo.lcap) {
            if (lane == 0) *wo.cold->overflow = 1u;
            wo.cur = kNoSpace;
            return kNoSpace;
        }
        wo.produced += need;
        return base;
    }
    if (wo.fill + need > kChunk) {
        const WaveOutCold k = *wo.cold;
        if (lane == 0) k.counts[wo.cur] = wo.fill;
        uint32_t c = 0;
        if (lane == 0) c = atomicAdd(k.nchunks, 1u);
        c = uniform(c) + k.nwaves;
        if (c >= k.max_chunks) {
            if (lane == 0) *k.overflow = 1u;
            wo.cur = kNoSpace;
            return kNoSpace;
        }
        wo.cur = c;
        wo.fill = 0;
    }
    const uint32_t base = wo.cur * kChunk + wo.fill;
    wo.fill += need;
    wo.produced += need;
    return base;
}

// Gathers address their tables as `scalar base + 32-bit byte offset` (global_load ... v_off, s[base:base+1]): one address VGPR
// per load in flight instead of a 64-bit pair.  The host guarantees every snapshot array and frontier buffer stays below
// 4 GiB (plan.cpp / alloc_frontier fail loudly beyond), which is > 1 G relationships per sorted array.
// Round 6: both say GLOBAL address space out loud.  The frontier buffers reach the walk through a two-element pointer array indexed by the level's
// parity, which loses the compiler's address-space inference: every entry load and store of the single-launch walk was a FLAT instruction (195 of
// them in the wide kernel's ISA) -- a flat access counts on lgkmcnt as well as vmcnt, so every LDS wait behind one waits for global memory too.
#if defined(__HIP_DEVICE_COMPILE__)
#define ACL_GLOBAL __attribute__((address_space(1)))
#else
#define ACL_GLOBAL  // (the host pass only parses these)
#endif
template <typename T>
__device__ __forceinline__ T gld(const T *__restrict__ base, uint32_t idx) {
    return *(const ACL_GLOBAL T *)((const ACL_GLOBAL char *)base + (uint32_t)(idx * (uint32_t)sizeof(T)));
}
template <typename T>
__device__ __forceinline__ void gst(T *__restrict__ base, uint32_t idx, const T &v) {
    *(ACL_GLOBAL T *)((ACL_GLOBAL char *)base + (uint32_t)(idx * (uint32_t)sizeof(T))) = v;
}

// Frontier entries of the single-launch walk are 8 BYTES (round 4; VERDICT r3 next #1b): the subject id and the subject key are constants of
// the REQUEST, so they live once per request in the block's LDS (s_req) and an entry keeps only what is its own:
//   x = object id[0:31) | probed[31]        y = slot[0:13) | level[13:19) | request index inside the unit[19:32)
// -- half the frontier bytes written, read back and kept in the L2, and a dwordx2 instead of a dwordx4 per lane and level.  Entries are
// decoded into the 16-byte register form (id, request, meta, subject id) right behind the load and encoded at the store: nothing else in
// process_segment knows.  The level loop (k_expand: requests of a whole batch, chunks shared by all waves) and the combine instantiations
// (entries name result CELLS, not requests) keep the 16-byte form.
template <bool E8>
__device__ __forceinline__ void put_entry(const WaveOut &wo, uint32_t idx, uint32_t id, uint32_t req, uint32_t meta, uint32_t sid) {
    if (E8) gst(reinterpret_cast<uint2 *>(wo.buf), idx, make_uint2(id | (((meta >> 19) & 1u) << 31), (meta & 0x7FFFFu) | ((req - wo.first) << 19)));
    else gst(wo.buf, idx, make_uint4(id, req, meta, sid));
}
// ... and the requests' answer bytes (has[] / err[]) of such a walk live in the block's LDS too, indexed by the request's place in the unit: the
// "is this request answered yet" read per entry and every hit / depth-error store are LDS accesses, not gathers and scattered byte stores in
// global memory (one of the ~6 vector-L1 line accesses per entry; each byte store was a 32 B write-through).  A: the array (LDS when L).
template <bool L>
__device__ __forceinline__ uint32_t ans_get(const uint8_t *a, uint32_t req, uint32_t first) {
    return L ? (uint32_t)a[req - first] : (uint32_t)gld(a, req);
}
template <bool L>
__device__ __forceinline__ void ans_set(uint8_t *a, uint32_t req, uint32_t first, uint8_t v) {
    if (L) a[req - first] = v;
    else a[req] = v;
}
__device__ __forceinline__ uint4 decode_entry8(const uint2 &v, const uint2 *sreq, uint32_t first) {
    const uint32_t rl = v.y >> 19;
    const uint2 rq = sreq[rl];  // {subject id, subject key}
    return make_uint4(v.x & 0x7FFFFFFFu, first + rl, (v.y & 0x7FFFFu) | ((v.x >> 31) << 19) | (rq.y << 20), rq.x);
}

// sorted sub-row (ids ascending; bit 31 of an edge is the leaf flag, not part of the id)
__device__ __forceinline__ bool row_contains(const uint32_t *__restrict__ edges, uint32_t lo, uint32_t hi, uint32_t key) {
    uint32_t end = hi;
    while (lo < hi) {
        uint32_t mid = (lo + hi) >> 1;
        if ((gld(edges, mid) & kIdMask) < key) lo = mid + 1;
        else hi = mid;
    }
    return lo < end && (gld(edges, lo) & kIdMask) == key;
}

// hashed row (plan.hpp): buckets of 4 ids; a SEEDED single-choice row keeps an id in bucket hrow_bucket(id, y) or nowhere -- ONE 16 B gather per
// membership test (round 5; rounds 1-4 placed every row two-choice: two gathers per test, and the walk's time follows the number of gather
// instructions its waves issue, profiles/r04_bucket_gather_sensitivity.txt) -- and a two-choice row (kRowTwoBit: a long row no seed was found
// for) in bucket h1 or h2: two independent gathers, never a probing chain.
// is `want` one of the four ids of a bucket?  Written as xor + min3: 4 v_xor + v_min3 + v_min + v_cmp (the obvious `p.x == want || ...`
// compiles to a chain of compares and i1 packing; the deep levels of a large batch are sensitive to VALU issue, profiles/r02_pmc_issue_breakdown.txt).
__device__ __forceinline__ bool bucket_has(const uint4 &p, uint32_t want) {
    return min(min(min(p.x ^ want, p.y ^ want), p.z ^ want), p.w ^ want) == 0u;
}
__device__ __forceinline__ bool bucket_row_contains(const uint4 *__restrict__ buckets, uint32_t b0, uint32_t y, uint32_t want) {
    const uint32_t h1 = hrow_bucket(want, y);
    bool hit = bucket_has(gld(buckets, b0 + h1), want);
    if (y & kRowTwoBit) hit = hit || bucket_has(gld(buckets, b0 + hrow_bucket2(want, y, h1)), want);
    return hit;
}

// Membership of (resource id, subject sid) in a membership-only class.  The class is stored SUBJECT-indexed:
// one hashed row of resource ids per subject.  All pending sub-checks of one request share the subject, so the
// lanes of a wave (which hold a few requests' worth of neighbouring entries) keep hitting the same descriptor
// and the same few bucket lines instead of 64 different resource rows.
__device__ __forceinline__ bool subject_row_contains(const DevGraph &g, const FwdOp &op, uint32_t id, uint32_t sid) {
    if (op.flags & OP_WILD) sid = op.K;  // `T:*`: the wildcard subject's row, whoever asks (the fast paths only take plain OP_PROBE_HASH programs)
    if (sid >= op.nrows) return false;
    const uint2 md = gld(reinterpret_cast<const uint2 *>(g.meta), op.base + sid);
    return md.y != 0u && bucket_row_contains(reinterpret_cast<const uint4 *>(g.buckets), md.x, md.y, id);
}

// Row descriptor {start, end} of (object id, sorted class op.k).  Relations with two sorted classes keep both
// descriptors in one aligned 16 B record: the state's second op re-reads the same line (an L1 hit) rather than carrying
// the record in five VGPRs across the expansions -- that cache was what kept the kernel above 96 VGPRs.
__device__ __forceinline__ uint2 row_meta(const DevGraph &g, const FwdOp &op, uint32_t id) {
    if (op.K == 2) {
        const uint4 v = gld(reinterpret_cast<const uint4 *>(g.meta), (op.base >> 1) + id);
        return op.k ? make_uint2(v.z, v.w) : make_uint2(v.x, v.y);
    }
    return gld(reinterpret_cast<const uint2 *>(g.meta), op.base + id * op.K + op.k);
}

// ---- combine programs (rewrites with `&` / `-`; plan.hpp SlotProg::combine).  A visited state with such a program gets `nleaves` fresh result
// cells (bytes of has[] / err[] behind the requests' own) and a CombineNode; its ops answer those cells exactly as a monotone walk answers a
// request; when the walk is over the nodes are evaluated deepest iteration first (resolve_node).  Everything here is compiled only into the
// CMB instantiations: the monotone kernels carry none of it.
struct CombineOut {  // (wave-uniform)
    uint4 *nodes = nullptr;                        // the region this walk appends to
    uint32_t *nnode = nullptr, *ncell = nullptr;   // its counters: LDS (single launch) or the status block (level loop)
    uint32_t node_cap = 0, cell_cap = 0, cell0 = 0;  // cell0: index of the region's first cell in has[] / err[]
    uint32_t iter = 0;                             // frontier iteration being processed
    const uint32_t *bexpr = nullptr;
};
enum : uint32_t { V_NO = 0u, V_HAS = 1u, V_ERR = 2u };
__device__ __forceinline__ uint32_t cell_value(const uint8_t *has, const uint8_t *err, uint32_t c) {
    const uint32_t h = __hip_atomic_load(has + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    const uint32_t e = __hip_atomic_load(err + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return h ? V_HAS : (e ? V_ERR : V_NO);
}
// value stack: two bits per value in one 64-bit register (<= kMaxLeaves values)
__device__ __forceinline__ void resolve_node(const uint4 &nd, const SlotProg *progs, const uint32_t *__restrict__ bexpr, uint8_t *has, uint8_t *err) {
    const SlotProg p = progs[nd.z & 0xFFFFu];
    const uint32_t *be = bexpr + p.combine;
    const uint32_t ntok = be[0];
    const uint32_t *tok = be + 2 + p.nleaves;
    unsigned long long st = 0;
    for (uint32_t i = 0; i < ntok; i++) {
        const uint32_t t = tok[i], kind = t & 0xFF000000u, arg = t & 0xFFFFFFu;
        uint32_t v;
        if (kind == BX_LEAF) {
            v = cell_value(has, err, nd.y + arg - 1u);
        } else if (kind == BX_LEAF_ALL) {  // a.all(b): folded from the children's cells by the member nodes (resolve_member)
            const uint32_t c = nd.y + arg - 1u;
            const uint32_t h = __hip_atomic_load(has + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP), e = __hip_atomic_load(err + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            v = (e & kAllNoBit) ? V_NO : ((e & 0x7Fu) ? V_ERR : (h ? V_HAS : V_NO));
        } else if (kind == BX_EXCL) {
            const uint32_t sub = (uint32_t)st & 3u, base = (uint32_t)(st >> 2) & 3u;
            st >>= 4;
            v = base != V_HAS ? base : (sub == V_ERR ? V_ERR : (sub == V_HAS ? V_NO : V_HAS));
        } else {  // BX_OR: HAS > ERR > NO; BX_AND: NO > ERR > HAS
            bool any_has = false, any_err = false, any_no = false;
            for (uint32_t k = 0; k < arg; k++) {
                const uint32_t x = (uint32_t)st & 3u;
                st >>= 2;
                any_has |= x == V_HAS;
                any_err |= x == V_ERR;
                any_no |= x == V_NO;
            }
            v = kind == BX_OR ? (any_has ? V_HAS : (any_err ? V_ERR : V_NO)) : (any_no ? V_NO : (any_err ? V_ERR : V_HAS));
        }
        st = (st << 2) | v;
    }
    const uint32_t v = ntok ? ((uint32_t)st & 3u) : V_NO;
    if (v == V_HAS) has[nd.x] = 1;
    else if (v == V_ERR) err[nd.x] = ITEM_ERR_DEPTH;
}
// member node of an intersection arrow {x: the arrow's leaf cell, y: the child's own cell, z: iteration << 16, w: 1}: the child's verdict is folded
// into the leaf cell -- HAS: "some child holds it"; NO / ERR: bits of the err byte, set with a word-wide atomic OR (several members of one
// arrow resolve at once; the neighbouring bytes' bits stay what they are).  Resolved BEFORE the regular nodes of its iteration.
__device__ __forceinline__ void resolve_member(const uint4 &nd, uint8_t *has, uint8_t *err) {
    const uint32_t v = cell_value(has, err, nd.y);
    if (v == V_HAS) {
        has[nd.x] = 1;
        return;
    }
    uint8_t *p = err + nd.x;
    const uint32_t sh = 8u * (uint32_t)((uintptr_t)p & 3u);
    atomicOr(reinterpret_cast<unsigned int *>((uintptr_t)p & ~(uintptr_t)3), (uint32_t)(v == V_NO ? kAllNoBit : ITEM_ERR_DEPTH) << sh);
}

// Child mode: evaluate every probe of state (slot, id) at `level` for subject (key, sid) without creating tasks.
// Returns true when the state still has something to enumerate (=> it must be written to the frontier).
// `leaf_known`: the edge that produced this child carried an authoritative leaf flag (`leaf`), so the child's
// own rows need not be looked at -- a plain-subject child then touches only the request subject's rows.
__device__ __forceinline__ bool eval_child(const DevGraph &g, const SlotProg *progs, const FwdOp *ops, uint32_t slot, uint32_t level, uint32_t key,
                                           uint32_t id, uint32_t sid, bool leaf_known, bool leaf, bool &hit, bool &depth_err) {
    const SlotProg p = progs[slot];
    if (level + p.max_dlevel > kMaxLevels) depth_err = true;
    const bool userset_subject = key < g.nslots;
    // plain subjects with a known leaf flag only need the probe-only ops
    const uint32_t nops = userset_subject ? p.n_total : (leaf_known ? p.n_probe : p.n_main);
    bool push = leaf_known && !leaf;
    for (uint32_t j = 0; j < nops; j++) {
        const FwdOp op = ops[p.first + j];
        const uint32_t L = level + op.dlevel;
        if (L > kMaxLevels) continue;
        if (op.flags & OP_REFLEX) {
            if (key == op.key && id == sid) hit = true;
        } else if (op.flags & OP_PUSH_SAME) {
            push = true;
        } else if (op.flags & OP_PROBE_HASH) {
            if (key == op.key) hit |= subject_row_contains(g, op, id, sid);
        } else if (id < op.nrows) {
            const bool probe = (op.flags & OP_PROBE) && key == op.key;
            const bool look = (op.flags & OP_ENUM) && !leaf_known;
            if (probe || look) {
                const uint2 md = row_meta(g, op, id);
                if (md.y > md.x) {
                    if (probe) hit |= row_contains(g.edges, md.x, md.y, sid);
                    if (look) push = true;
                }
            }
        }
    }
    return push;
}

// Fast path of the expansion for the shape that dominates deep levels: every task's child state is "simple" -- one hashed
// probe of the request's subject (a plain subject) plus an authoritative leaf flag on the edge, nothing else -- and all
// tasks agree on (child slot, subject key).  Then there is no program to interpret, and each lane evaluates kSimpleWidth children
// per step with branch-free loads (dummy in-range addresses for inactive lanes), so the edge, descriptor and bucket
// gathers of 64 x kSimpleWidth children are in flight together instead of 64 at a time behind three dependent waits.
// Bit-for-bit the same decisions, the same output entries in the same order as the generic path.
#ifndef ACL_ISA_NO_SLOW
#define ACL_ISA_NO_SLOW 0  // 1: tools/isa_loops.py only -- the simple expansion WITHOUT its rare slow-row block, so that the static instruction counts are the main path's (never run)
#endif
#ifndef ACL_SIMPLE_WIDTH
#define ACL_SIMPLE_WIDTH 3  // children per lane and step.  Round 5: with ONE bucket per child three of them cost the registers two used to, and the wide walk moved to 12 waves per
                            // block = 6 per SIMD = room for 72 VGPRs without a spill (rounds 2-4: 2 at 64 VGPRs and 8 waves per SIMD); profiles/r05_ab_block_shape.txt
#endif
constexpr int kSimpleWidth = ACL_SIMPLE_WIDTH;  // children per lane whose buckets are in flight together
// Returns a bit mask of the 64-task rounds it did NOT handle (the caller expands those the generic way): a round whose rows
// together exceed the head-bit window (a row of thousands of ids) or with a task at the dispatch-depth limit.
//
// Instruction count is what bounds this loop (the deep levels of a large batch keep the vector ALU busy 60 % of the launch,
// profiles/r02_pmc_issue_breakdown.txt), so everything that is a property of the TASK is done once per task, not per child:
//   - the subject's row {first bucket, count} sits in the task (DESC: fetched by the parent lane together with its has[] byte
//     and row descriptor; otherwise fetched here, one gather per 64 tasks) -- no per-child descriptor gather;
//   - depth limits are checked per task (above);
//   - work item -> task without a search: every task owns >= 1 consecutive work items, so task lanes set ONE head bit each
//     (LDS atomic or) at their first work item; a lane's task is then `tasks before this 64-item window` + the head bits at or
//     below its lane (two v_mbcnt) -- the 6-step binary search over the LDS prefix array cost ~30 VALU + 6 LDS reads per child;
//   - one output reservation per step for the W x 64 children, not one per 64.
// The steps of the simple expansion: the wave's task list holds T tasks whose children are `total` work items, t.a[j].x = first edge minus first work
// item, t.heads = one bit per task at its first work item (set by the caller's prologue).  UM: every child carries the same meta `umeta`, the
// entries are 8-byte ones (no per-task meta / subject id reads at the push) and t.a[j].w is the request's index INSIDE the unit (the answer-byte
// accesses and the entry's y word without their subtractions).
// PT (with UM; states of the two-hop slot, plan.hpp Snapshot::hop2_*): the children's level travels PER TASK -- t.a[j].w = request index << 19 | child level << 13,
// `umeta` is the child slot alone and an entry's y word is their sum; hopadd = 1 << 13 while the tasks name two-hop rows, else 0: an edge with kHop2Bit is a
// grandchild -- bit 30 is not part of its id, and its state lies one level further on.  Every other expansion is instantiated without any of it.
// One step: N (<= kSimpleWidth) windows of 64 children from work item w0 on.  Their edges go out in one trip (one VGPR each), then their buckets
// (8 VGPRs per child).  What the walk's time follows is the number of vector-memory INSTRUCTIONS its waves issue, whatever the number of lanes
// that need them (profiles/r04_bucket_gather_sensitivity.txt, r06_ab_check_local.txt `warm`): a window without a valid lane costs what a full one
// costs, so the LAST step of an expansion is instantiated only as wide as its children (simple_steps) -- every body keeps the shape: all edge loads,
// fence, all bucket loads, fence, compares, stores behind the last compare.
template <bool LOCAL, bool E8, bool UM, int N, bool PT = false>
__device__ __forceinline__ void simple_step(TaskLds &t, uint32_t w0, uint32_t total, uint32_t &before, WaveOut &wo, uint32_t lane, const uint32_t *__restrict__ edges,
                                            const uint4 *__restrict__ buckets, uint8_t *has, uint8_t *err, uint32_t umeta, uint32_t hopadd = 0u) {
    static_assert(!PT || UM, "per-task levels ride in the uniform-meta form's task word");
    const uint32_t idm = PT ? (kIdMask ^ (hopadd << 17)) : kIdMask;  // (uniform: without kHop2Bit while two-hop rows are read)
    bool valid[N];
    uint32_t tj[N], edge[N];
#pragma unroll
    for (int k = 0; k < N; k++) {
        const uint32_t win = (w0 >> 6) + (uint32_t)k;
        const uint64_t hw = win < kHeadWords ? t.heads[win] : 0ull;
        const uint32_t hlo = uniform((uint32_t)hw), hhi = uniform((uint32_t)(hw >> 32));
        const uint32_t w = w0 + 64u * k + lane;
        valid[k] = w < total;
        const uint32_t wv = valid[k] ? w : total - 1;  // inactive lanes shadow the last child: every load stays in range
        // tasks starting at or before this lane's work item, minus one (beyond `total` there are no head bits: the last task)
        // (the lane's own head bit straight from the uniform mask -- inverse ballot: the mask IS the condition register; `(hw >> lane) & 1` is a 64-bit
        //  vector shift, quarter rate, plus an AND per child window)
        const uint32_t own = __builtin_amdgcn_inverse_ballot_w64(((uint64_t)hhi << 32) | hlo) ? 1u : 0u;
        const uint32_t j = before + __builtin_amdgcn_mbcnt_hi(hhi, __builtin_amdgcn_mbcnt_lo(hlo, 0u)) + own - 1u;
        before += (uint32_t)__popc(hlo) + (uint32_t)__popc(hhi);
        tj[k] = j;
        edge[k] = gld(edges, t.a[j].x + wv);
    }
    issue_fence();  // trip 1: every edge of the step
    ACL_MARK(wo, PH_EDGES);
    uint4 p[N];
    uint32_t rq[N];
    uint32_t slow = 0u;
#pragma unroll
    for (int k = 0; k < N; k++) {
        const uint4 ta = t.a[tj[k]];  // the child's task: {edge base, first bucket, the row's y (buckets | two-choice | seed), request} in one 16-byte read
        rq[k] = ta.w;
        // (hrow_fast: full-rate arithmetic, in range for EVERY row and right for all but the slow ones -- those are redone below)
        p[k] = gld(buckets, ta.y + hrow_fast(edge[k] & idm, ta.z));
        slow |= ta.z;
    }
    issue_fence();  // trip 2: the N buckets
    ACL_MARK(wo, PH_BUCKETS);
    bool hit[N], push[N];
    uint64_t pb[N];
    uint32_t pre[N], np = 0;
#pragma unroll
    for (int k = 0; k < N; k++) hit[k] = valid[k] & bucket_has(p[k], edge[k] & idm);
    if (!ACL_ISA_NO_SLOW && __ballot(hrow_is_slow(slow))) {  // (rare: a child whose request's subject has a SLOW row -- two-choice, or 2^16 buckets and more: its bucket(s) by the
                                         //  32-bit hash, one child at a time; a hit in the fast hash's bucket of such a row is still a hit: the id IS in the row)
#pragma unroll
        for (int k = 0; k < N; k++) {
            const uint4 ta = t.a[tj[k]];
            if (hrow_is_slow(ta.z)) {
                const uint32_t cid = edge[k] & idm, h1 = hrow_slow(cid, ta.z);
                uint4 q = gld(buckets, ta.y + h1);
                bool h = bucket_has(q, cid);
                if (ta.z & kRowTwoBit) {
                    q = gld(buckets, ta.y + hrow_bucket2(cid, ta.z, h1));
                    h = h | bucket_has(q, cid);
                }
                hit[k] = hit[k] | (valid[k] & h);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < N; k++) {
        // (bitwise, not &&: a short-circuit puts the compare under a branch, and the compiler then waits for "maybe still pending"
        //  loads at the end of every step; depth limits were checked per task above)
        push[k] = valid[k] & !hit[k] & ((edge[k] & kLeafBit) == 0u);
    }
    // stores only after the last compare: a conditional store between two compares makes the second one's wait cover it
    // (vmcnt counts stores too, and the compiler must assume the store was not issued)
    {
        // (one branch for the step's hits, not an exec-mask round trip per child: most steps of the deep levels answer nobody)
        bool anyhit = hit[0];
#pragma unroll
        for (int k = 1; k < N; k++) anyhit = anyhit | hit[k];
        if (__ballot(anyhit)) {
#pragma unroll
            for (int k = 0; k < N; k++)
                if (hit[k]) ans_set<E8>(has, PT ? rq[k] >> 19 : rq[k], UM ? 0u : wo.first, 1);
        }
    }
    if (E8) {
        // a request answered by THIS step's hits (or by another wave a moment ago) needs none of its other children any more: looked at
        // once more before they are written -- an entry not written is not read back, and frees a lane of a segment of the next level
        // (C4 253 -> 238 us; profiles/r04_push_recheck_ab.txt)
        wave_lds_fence();
        uint32_t hv[N];  // (the N answer bytes travel together: one LDS round trip, not N dependent ones)
#pragma unroll
        for (int k = 0; k < N; k++) hv[k] = ans_get<true>(has, PT ? rq[k] >> 19 : rq[k], UM ? 0u : wo.first);
        issue_fence();
#pragma unroll
        for (int k = 0; k < N; k++) push[k] = push[k] & (hv[k] == 0u);
    }
#pragma unroll
    for (int k = 0; k < N; k++) {
        pb[k] = __ballot(push[k]);
        pre[k] = np;
        np += (uint32_t)__popcll(pb[k]);
    }
    if (np) {
        const uint32_t base = reserve<LOCAL>(wo, np, lane);
        if (base != kNoSpace) {
#pragma unroll
            for (int k = 0; k < N; k++)
                if (push[k]) {
                    if (PT)  // (the task holds the entry's request and level bits; a grandchild's extra level is added)
                        gst(reinterpret_cast<uint2 *>(wo.buf), base + pre[k] + lanes_below(pb[k]), make_uint2((edge[k] & idm) | 0x80000000u, umeta + rq[k] + ((edge[k] >> 17) & hopadd)));
                    else if (UM)  // (the task holds the request's index inside the unit: the entry's y word without the subtraction)
                        gst(reinterpret_cast<uint2 *>(wo.buf), base + pre[k] + lanes_below(pb[k]), make_uint2((edge[k] & kIdMask) | 0x80000000u, (umeta & 0x7FFFFu) | (rq[k] << 19)));
                    else
                        put_entry<E8>(wo, base + pre[k] + lanes_below(pb[k]), edge[k] & kIdMask, rq[k], (UM ? umeta : t.meta[tj[k]]) | kProbedBit, UM ? 0u : t.sid[tj[k]]);
                }
        }
    }
#if ACL_PROFILE_PHASES  // (instrumented builds: steps issued, and the windows a full-width step would have issued for no valid lane)
    if (lane == 0) {
        wo.cold->prof[16] += 1u;
        wo.cold->prof[17] += (uint32_t)(kSimpleWidth - N);
    }
#endif
    ACL_MARK(wo, PH_PUSH);
}
template <bool LOCAL, bool E8, bool UM, bool PT = false>
__device__ __forceinline__ void simple_steps(TaskLds &t, uint32_t total, WaveOut &wo, uint32_t lane, const uint32_t *__restrict__ edges, const uint4 *__restrict__ buckets,
                                             uint8_t *has, uint8_t *err, uint32_t umeta, uint32_t hopadd = 0u) {
    constexpr int W = kSimpleWidth;
    static_assert(W == 3, "the step bodies below are the widths 1 .. 3");
    uint32_t before = 0;  // tasks that start before the current 64-item window
    ACL_MARK(wo, PH_PROLOGUE);
    for (uint32_t w0 = 0; w0 < total; w0 += 64 * W) {
        const uint32_t left = total - w0;  // (uniform: one branch per step)
        if (!E8 || left > 128u) simple_step<LOCAL, E8, UM, 3, PT>(t, w0, total, before, wo, lane, edges, buckets, has, err, umeta, hopadd);
        else if (left > 64u) simple_step<LOCAL, E8, UM, 2, PT>(t, w0, total, before, wo, lane, edges, buckets, has, err, umeta, hopadd);
        else simple_step<LOCAL, E8, UM, 1, PT>(t, w0, total, before, wo, lane, edges, buckets, has, err, umeta, hopadd);
    }
}

template <bool SHARDED, bool LOCAL, bool DESC, bool E8>
__device__ __forceinline__ uint32_t flush_simple(TaskLds &t, uint32_t T, WaveOut &wo, uint32_t lane, const DevGraph &g, const SlotProg &cp, const FwdOp &pop,
                                                  uint8_t *has, uint8_t *err) {
    const uint32_t *__restrict__ edges = g.edges;
    const uint4 *__restrict__ buckets = reinterpret_cast<const uint4 *>(g.buckets);
    uint32_t skipped = 0;
    // ONE round for the whole list (<= kTaskCap = 128 tasks): every lane owns tasks `lane` and `64 + lane`.  Two rounds of 64 paid this
    // prologue -- a chain of dependent LDS round trips: counts, scan, head bits, fences -- twice per pair of segments
    // (17 % of the walk's wave-time, profiles/r02_walk_phase_breakdown.txt).
    {
        const bool mine0 = lane < T, mine1 = 64u + lane < T;
        const uint32_t cnt0 = mine0 ? (t.count[lane] & kCountMask) : 0u, cnt1 = mine1 ? (t.count[64u + lane] & kCountMask) : 0u;
        const uint32_t incl0 = wave_incl_scan(cnt0, lane);
        const uint32_t tot0 = wave_last(incl0);
        const uint32_t incl1 = wave_incl_scan(cnt1, lane) + tot0;
        const uint32_t total = wave_last(incl1);
        const uint32_t lvl0 = mine0 ? meta_level(t.meta[lane]) : 0u, lvl1 = mine1 ? meta_level(t.meta[64u + lane]) : 0u;
        const uint32_t lvl = max(lvl0, lvl1);
        if (total > 64u * kHeadWords || __ballot(lvl + pop.dlevel > kMaxLevels || lvl + cp.max_dlevel > kMaxLevels)) return ~0u;
        const uint32_t excl0 = incl0 - cnt0, excl1 = incl1 - cnt1;
        if (!DESC) {
#pragma unroll
            for (uint32_t h = 0; h < 2; h++) {
                const uint32_t i = h * 64u + lane;
                if (i < T) {
                    const uint32_t sidt = t.sid[i];
                    const uint2 d = gld(reinterpret_cast<const uint2 *>(g.meta), pop.base + (sidt < pop.nrows ? sidt : 0u));
                    const bool row = sidt < pop.nrows && d.y != 0u;
                    t.a[i].y = row ? d.x : 0u;
                    t.a[i].z = row ? d.y : 1u;  // (the row's y: buckets | two-choice | seed; {0, 1} = the reserved empty bucket)
                }
            }
        }
        // (t.heads is all zero here: zeroed at kernel start and behind every expansion)
        // first edge of the task minus its first work item: edge index = this + work item
        if (mine0) t.a[lane].x -= excl0;
        if (mine1) t.a[64u + lane].x -= excl1;
        if (mine0) atomicOr(reinterpret_cast<unsigned long long *>(&t.heads[excl0 >> 6]), 1ull << (excl0 & 63u));
        if (mine1) atomicOr(reinterpret_cast<unsigned long long *>(&t.heads[excl1 >> 6]), 1ull << (excl1 & 63u));
        wave_lds_fence();
        simple_steps<LOCAL, E8, false>(t, total, wo, lane, edges, buckets, has, err, 0u);
        if (lane < kHeadWords) t.heads[lane] = 0ull;  // (left zero for the next expansion: one LDS round trip less in its prologue)
        wave_lds_fence();
    }
    return skipped;
}

// Second specialised expansion: all tasks lead to one child slot whose program is at most two hashed probes followed by at
// most two enumerate ops that a child is only LOOKED at for ("does it have anything to enumerate?") -- arrow targets such as
// `namespace#view = viewer + creator + ...`.  One child per lane; the subject's row descriptors (they depend on the request,
// not on the child) are fetched together with the edge, then every bucket and every row descriptor of the child together:
// two dependent trips instead of up to six.  Same decisions and output order as the generic path.
template <bool SHARDED, bool LOCAL, bool E8>
__device__ __forceinline__ void flush_probes(TaskLds &t, uint32_t T, WaveOut &wo, uint32_t lane, const DevGraph &g, const SlotProg &cp, const FwdOp *cops,
                                             uint32_t k0, bool leafauth, uint8_t *has, uint8_t *err) {
    const uint32_t *__restrict__ edges = g.edges;
    const uint2 *__restrict__ meta2 = reinterpret_cast<const uint2 *>(g.meta);
    const uint4 *__restrict__ buckets = reinterpret_cast<const uint4 *>(g.buckets);
    const uint32_t nh = uniform(cp.n_probe), nl = leafauth ? 0u : uniform(cp.n_main - cp.n_probe);
    const FwdOp *lops = cops + cp.n_probe;
    for (uint32_t gq = 0; gq < T; gq += 64) {
        const uint32_t cnt = (gq + lane < T) ? (t.count[gq + lane] & kCountMask) : 0u;
        const uint32_t incl = wave_incl_scan(cnt, lane);
        const uint32_t total = wave_last(incl);
        t.scan[lane] = incl - cnt;
        wave_lds_fence();
        for (uint32_t w0 = 0; w0 < total; w0 += 64) {
            const uint32_t w = w0 + lane;
            const bool valid = w < total;
            const uint32_t wv = valid ? w : total - 1;  // inactive lanes shadow the last child: every load stays in range
            uint32_t j = 0;
#pragma unroll
            for (uint32_t step = 32; step >= 1; step >>= 1)
                if (t.scan[j + step] <= wv) j += step;
            const uint32_t tj = gq + j;
            const uint32_t sid = t.sid[tj];
            const uint32_t level = meta_level(t.meta[tj]);
            // trip 1: the edge and the subject's row descriptor of every probe
            const uint32_t edge = gld(edges, t.a[tj].x + (wv - t.scan[j]));
            uint2 hd[2];
            bool hrow[2];
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const bool hk = (uint32_t)k < nh;
                hrow[k] = hk && cops[hk ? k : 0].key == k0 && sid < cops[hk ? k : 0].nrows;
                hd[k] = gld(meta2, (hk ? cops[k].base : 0u) + (hrow[k] ? sid : 0u));
            }
            const uint32_t child = edge & kIdMask;
            // trips 2 and 3: the bucket of the first probe, then of the second (two-probe programs only), one after the other (register budget)
            bool hit = false, push = leafauth && !(edge & kLeafBit);
            auto probe = [&](const uint2 &hdk, bool hrk, uint32_t dl) {
                const bool hr = hrk && hdk.y != 0u;
                const uint32_t b0 = hr ? hdk.x : 0u, y = hr ? hdk.y : 1u;  // (no row: the reserved empty bucket)
                const uint4 bp = gld(buckets, b0 + hrow_fast(child, y));  // (in range for every row, right for the fast ones)
                bool h = bucket_has(bp, child);
                if (__ballot(hrow_is_slow(y))) {  // (rare: two-choice rows and rows of 2^16 buckets and more)
                    if (hrow_is_slow(y)) {
                        const uint32_t h1 = hrow_slow(child, y);
                        h = h || bucket_has(gld(buckets, b0 + h1), child);
                        if (y & kRowTwoBit) h = h || bucket_has(gld(buckets, b0 + hrow_bucket2(child, y, h1)), child);
                    }
                }
                if (hr && level + dl <= kMaxLevels) hit = hit || h;
            };
            if (nh > 0) probe(hd[0], hrow[0], cops[0].dlevel);
            asm volatile("" ::: "memory");  // keep the second probe's gathers behind the first's (register budget, see above)
            if (nh > 1) probe(hd[1], hrow[1], cops[1].dlevel);
            asm volatile("" ::: "memory");
            // the child's own rows are looked at only where the edge carries no authoritative leaf flag (after a patch
            // made an op distrust them): one more trip, rare
            if (nl) {
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    const bool lk = (uint32_t)k < nl;
                    const FwdOp &lo = lops[lk ? k : 0];
                    const bool inrow = lk && child < lo.nrows;
                    const uint2 md = gld(meta2, lk ? lo.base + (inrow ? child : 0u) * lo.K + lo.k : 0u);
                    if (inrow && md.y > md.x && level + lo.dlevel <= kMaxLevels) push = true;
                }
            }
            const uint32_t req = t.a[tj].w, meta = t.meta[tj];
            hit = hit && valid;
            push = push && valid;
            if (hit) {
                ans_set<E8>(has, req, wo.first, 1);
                push = false;
            } else if (valid && level + cp.max_dlevel > kMaxLevels) {
                ans_set<E8>(err, req, wo.first, ITEM_ERR_DEPTH);
            }
            if (E8) {  // (as in flush_simple: a request answered meanwhile needs none of its other children)
                wave_lds_fence();
                push = push && ans_get<true>(has, req, wo.first) == 0u;
            }
            const uint64_t b = __ballot(push);
            if (b) {
                const uint32_t base = reserve<LOCAL>(wo, (uint32_t)__popcll(b), lane);
                if (push && base != kNoSpace) put_entry<E8>(wo, base + lanes_below(b), child, req, meta | kProbedBit, sid);
            }
        }
        wave_lds_fence();
    }
}

// Expand the first T tasks of the wave's LDS list.  INLINE: children are probed here and only the ones with
// remaining enumeration work are written (forward Check); otherwise every child is written (reverse walk).
// wave-cooperative append of the flagged lanes' entries to the shard's export buffer (one atomic per call and destination).
// sh.by_dest: one buffer per destination shard (`dest` = owner of the entry's slot) for an all-to-all exchange; otherwise
// one buffer that every shard receives (all-gather; also the reverse walk's broadcast of visited states).
__device__ __forceinline__ void export_entries(bool xport, const uint4 &e, uint32_t dest, uint32_t lane, const DevShard &sh) {
    uint64_t todo = __ballot(xport);
    if (!todo) return;
    if (!sh.by_dest) {
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(sh.exp_count, (uint32_t)__popcll(todo));
        const uint32_t at = uniform(base) + lanes_below(todo);
        if (xport && at < sh.cap) sh.exp[at] = e;
        return;
    }
    while (todo) {
        const uint32_t d = (uint32_t)__builtin_amdgcn_readlane((int)dest, (int)(__ffsll((unsigned long long)todo) - 1));
        const bool mine = xport && dest == d;
        const uint64_t m = __ballot(mine);
        todo &= ~m;
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(sh.exp_count + 1 + d, (uint32_t)__popcll(m));
        const uint32_t at = uniform(base) + lanes_below(m);
        if (mine && at < sh.cap) sh.exp[(size_t)d * (sh.stride ? sh.stride : sh.cap) + at] = e;
    }
}

template <bool INLINE, bool SHARDED, bool LOCAL, bool DESC = false, bool CMB = false>  // DESC: the tasks carry the subject's hashed row (TaskLds b0 / nb); CMB: child slots may hold combine programs
__device__ __forceinline__ void flush_tasks(TaskLds &t, uint32_t T, WaveOut &wo, uint32_t lane, const DevGraph &g, const SlotProg *progs,
                                            const FwdOp *ops, const uint32_t *__restrict__ edges, uint8_t *has, uint8_t *err, const DevShard &sh,
                                            bool same = false /* the caller made every task from ONE op: child slot, key and flags agree */,
                                            const CombineOut &co = CombineOut() /* CMB: where the children of an intersection arrow get their cells and member nodes */) {
    constexpr bool E8 = INLINE && LOCAL && !CMB;  // (8-byte entries: the single-launch walk's monotone instantiations)
    uint32_t only = ~0u;  // rounds of 64 tasks left for the generic loop
    wave_lds_fence();
    if (INLINE) {  // all tasks lead to the same "simple" child state?  (one hashed probe + authoritative leaf flags, plain subject)
        const uint32_t m0 = t.meta[0];
        const uint32_t cs = uniform(meta_slot(m0)), k0 = uniform(meta_key(m0));
        const SlotProg cp = progs[cs];
        bool ok = cp.n_probe == 1 && k0 >= g.nslots && (!SHARDED || cp.owner == sh.rank);
        FwdOp pop{};
        if (ok) {
            pop = ops[cp.first];
            ok = pop.flags == OP_PROBE_HASH && pop.key == k0;
        }
        bool agree = true;
        if (same) {
            agree = (t.count[0] & (kLeafAuthBit | kSelfBit)) == kLeafAuthBit;
        } else {
            for (uint32_t i = lane; i < T; i += 64) {
                const uint32_t mi = t.meta[i], ci = t.count[i];
                agree = agree && meta_slot(mi) == cs && meta_key(mi) == k0 && (ci & kLeafAuthBit) && !(ci & (kSelfBit | kAllBit));
            }
        }
        if (ok && !__ballot(!agree)) {
            only = flush_simple<SHARDED, LOCAL, DESC, E8>(t, T, wo, lane, g, cp, pop, has, err);
            if (!only) return;
        } else
        // second shape: <= 2 hashed probes + <= 2 enumerate ops that are only looked at; uniform slot, key and leaf authority
        if (k0 >= g.nslots && (!SHARDED || cp.owner == sh.rank) && cp.n_probe <= 2 && cp.n_main - cp.n_probe <= 2 && !(CMB && cp.combine)) {
            const FwdOp *cops = ops + cp.first;
            bool shape = true;
            for (uint32_t q = 0; q < cp.n_main; q++) {
                const uint32_t fl = cops[q].flags;
                shape = shape && (q < cp.n_probe ? fl == OP_PROBE_HASH : ((fl & OP_ENUM) && !(fl & (OP_PUSH_SAME | OP_REFLEX | OP_PROBE_HASH)) && cops[q].K != 2));
            }
            const bool la0 = (t.count[0] & kLeafAuthBit) != 0;
            bool agree2 = true;
            for (uint32_t i = lane; i < T; i += 64) {
                const uint32_t mi = t.meta[i], ci = t.count[i];
                agree2 = agree2 && meta_slot(mi) == cs && meta_key(mi) == k0 && ((ci & kLeafAuthBit) != 0) == la0 && !(ci & (kSelfBit | kAllBit));
            }
            if (shape && !__ballot(!agree2)) {
                flush_probes<SHARDED, LOCAL, E8>(t, T, wo, lane, g, cp, cops, k0, la0, has, err);
                return;
            }
        }
    }
    for (uint32_t gq = 0; gq < T; gq += 64) {
        if (!(only & (1u << (gq >> 6)))) continue;
        const uint32_t cnt = (gq + lane < T) ? (t.count[gq + lane] & kCountMask) : 0u;
        const uint32_t incl = wave_incl_scan(cnt, lane);
        const uint32_t total = wave_last(incl);
        t.scan[lane] = incl - cnt;
        wave_lds_fence();
        for (uint32_t w0 = 0; w0 < total; w0 += 64) {
            const uint32_t w = w0 + lane;
            bool push = false, xport = false, live = false, isall = false;
            uint4 e = make_uint4(0, 0, 0, 0);
            uint32_t c = 0, edge = 0, child = 0, s = 0, j = 0;
            if (w < total) {
                // largest j with scan[j] <= w
#pragma unroll
                for (uint32_t step = 32; step >= 1; step >>= 1)
                    if (t.scan[j + step] <= w) j += step;
                const uint32_t tj = gq + j;
                c = t.count[tj];
                s = t.a[tj].x;
                edge = (c & kSelfBit) ? s : gld(edges, s + (w - t.scan[j]));
                child = INLINE ? (edge & kIdMask) : edge;
                e = make_uint4(child, t.a[tj].w, t.meta[tj], t.sid[tj]);
                push = live = true;
                isall = CMB && (c & kAllBit);
            }
            if (CMB) {
                // children of an intersection arrow a.all(b): a result cell of its own for every child, and a member node that folds the child's
                // verdict into the arrow's leaf cell (resolve_member) -- one reservation per wave and window
                const uint64_t ab = __ballot(isall);
                if (ab) {
                    const uint32_t k = (uint32_t)__popcll(ab);
                    uint32_t c0 = 0, n0 = 0;
                    if (lane == 0) {
                        c0 = atomicAdd(co.ncell, k);
                        n0 = atomicAdd(co.nnode, k);
                    }
                    c0 = uniform(c0);
                    n0 = uniform(n0);
                    if (c0 + k > co.cell_cap || n0 + k > co.node_cap) {  // out of cells / nodes: as where a combine state is visited (process_segment)
                        if (LOCAL) {
                            if (lane == 0) *wo.cold->overflow = 1u;
                            wo.cur = kNoSpace;
                        } else if (lane == 0) {
                            *wo.cold->overflow = SHARDED ? kOverflowPools : 3u;
                        }
                        if (isall) push = live = false;
                    } else if (isall) {
                        const uint32_t r = lanes_below(ab), cell = co.cell0 + c0 + r;
                        has[cell] = 0;
                        err[cell] = ITEM_ERR_NONE;
                        co.nodes[n0 + r] = make_uint4(e.y, cell, co.iter << 16, 1u);
                        e.y = cell;
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  // (the zeroes are acknowledged before a probe of the child stores a hit)
                }
            }
            if (live) {
                if (INLINE && SHARDED && progs[meta_slot(e.z)].owner != sh.rank) {
                    // the child's rows live on another shard: it leaves unprobed and is evaluated by its owner
                    push = false;
                    xport = true;
                } else if (INLINE && CMB && progs[meta_slot(e.z)].combine) {
                    // a combine child is visited as a state of its own, unprobed: its probes answer leaf cells that only exist once it is
                } else if (INLINE) {
                    bool hit = false, derr = false;
                    push = eval_child(g, progs, ops, meta_slot(e.z), meta_level(e.z), meta_key(e.z), child, e.w, (c & kLeafAuthBit) != 0,
                                      (edge & kLeafBit) != 0, hit, derr);
                    if (hit) {
                        ans_set<E8>(has, e.y, wo.first, 1);
                        push = false;
                    } else if (derr) {
                        ans_set<E8>(err, e.y, wo.first, ITEM_ERR_DEPTH);
                    }
                    e.z |= kProbedBit;
                }
            }
            if (E8 && INLINE) {  // (as in flush_simple: a request answered meanwhile needs none of its other children)
                wave_lds_fence();
                push = push && ans_get<true>(has, e.y, wo.first) == 0u;
            }
            const uint64_t b = __ballot(push);
            if (b) {
                const uint32_t base = reserve<LOCAL>(wo, (uint32_t)__popcll(b), lane);
                if (push && base != kNoSpace) put_entry<E8>(wo, base + lanes_below(b), e.x, e.y, e.z, e.w);
            }
            if (INLINE && SHARDED) export_entries(xport, e, xport ? progs[meta_slot(e.z)].owner : 0u, lane, sh);
        }
        wave_lds_fence();
    }
}

// ------------------------------------------------------------------ seed
// items: acl_item_t (16 B): x = rtype | perm << 16, y = resource id, z = stype | srel << 16, w = subject id
__global__ __launch_bounds__(256) void k_seed(DevGraph g, DevFrontier f, const uint4 *__restrict__ items, uint32_t n, uint8_t *has, uint8_t *err,
                                              DevShard sh) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t need = (n + kChunk - 1) / kChunk;       // chunks holding seeds: ids [0, need)
    const uint32_t readable = max(need, f.nwaves);          // the reader scans every static chunk
    // status block = nchunks[kLevelSlots] | any[kLevelSlots] | overflow | export count, contiguous from f.nchunks:
    // reset here (no separate memset launch); slot 0 describes the seeds
    if (i < kStatusWords) f.nchunks[i] = i == 0 ? (need > f.nwaves ? need - f.nwaves : 0u) : (i == kLevelSlots ? 1u : 0u);
    if (i < readable) f.counts[0][i] = i < need ? min(kChunk, n - i * kChunk) : 0u;
    if (i >= n) return;
    uint4 it = items[i];
    uint32_t rtype = it.x & 0xFFFFu, perm = it.x >> 16, stype = it.z & 0xFFFFu, srel = it.z >> 16;
    bool ok = rtype < g.ntypes && stype < g.ntypes && perm < g.type_nmembers[rtype < g.ntypes ? rtype : 0] &&
              (srel == 0xFFFFu || srel < g.type_nmembers[stype < g.ntypes ? stype : 0]);
    has[i] = 0;
    err[i] = ok ? ITEM_ERR_NONE : ITEM_ERR_INVALID;
    uint32_t meta = kDeadMeta;
    if (ok) {
        uint32_t slot = g.type_slot_base[rtype] + perm;
        uint32_t key = srel == 0xFFFFu ? g.nslots + stype : g.type_slot_base[stype] + srel;
        meta = make_meta(slot, 1u, key);
        if (sh.world > 1 && g.progs[slot].owner != sh.rank) meta = kDeadMeta;  // seeded by the shard that owns the resource type
    }
    f.buf[0][i] = make_uint4(it.y, i, meta, it.w);
}

// reverse-walk seeds: lookup request i starts from subject sids[i]; entry meta = subject key (dist 0 => program rseeds[key]).
// Also resets the status block (slot 0 describes the seeds), like k_seed.
__global__ __launch_bounds__(256) void k_rev_seed(DevFrontier f, const uint32_t *__restrict__ sids, uint32_t n, uint32_t key) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t need = (n + kChunk - 1) / kChunk;
    const uint32_t readable = max(need, f.nwaves);
    if (i < kStatusWords) f.nchunks[i] = i == 0 ? (need > f.nwaves ? need - f.nwaves : 0u) : (i == kLevelSlots ? (n ? 1u : 0u) : 0u);
    if (i < readable) f.counts[0][i] = i < need ? min(kChunk, n - i * kChunk) : 0u;
    if (i < n) f.buf[0][i] = make_uint4(sids[i], i, key, 0);
}

// ---------------------------------------------------------------- expand
// One 64-entry segment of the frontier: every lane holds one pending sub-check.  Shared by the level-synchronous kernel
// (k_expand: segments come from the chunked global frontier) and the single-launch kernel (k_check_local: segments
// come from the wave's private region).  `next` lets the simple-parent fast path pull the following segment in early:
//   bool peek(uint4 &e, bool &valid)  loads the next segment's entries if there is one (not consumed yet)
//   void take()                       consumes it
template <bool SHARDED, bool LOCAL, bool CMB, typename Next, bool SEEDS = false /* the entries are a batch's seeds: never probed, so never "simple parents" -- the fast path is not compiled in */>
__device__ __forceinline__ void process_segment(const uint4 &e, bool valid, Next &next, TaskLds &t, WaveOut &wo, uint32_t lane, const DevGraph &g,
                                                const SlotProg *progs, const FwdOp *ops, uint8_t *has, uint8_t *err, const DevShard &sh,
                                                const CombineOut &co = CombineOut()) {
    constexpr bool E8 = LOCAL && !CMB;  // 8-byte entries + answers in LDS (put_entry, ans_get)
    const uint32_t id = e.x, req = e.y, meta = e.z;
    // ---- fast path: every entry of the segment is a "simple parent" -- probes already done by its own parent (kProbedBit),
    // plain subject, and a program whose only remaining op enumerates one sorted row.  No interpreter: the has[] read, the
    // row-descriptor gather and the subject's row of the child's probe are issued together (branch-free), for this segment (A)
    // and the wave's next one (B) at once.  The slots may differ from lane to lane (level 2 of a pod check holds `namespace#view`
    // and `group#member` states side by side): each lane reads ITS program from the LDS copy; a segment of one slot (the deep
    // levels) reads it once, through the scalar path.
    if (!__ballot(valid)) return;
    if (!SEEDS) {
        const uint64_t vb = __ballot(valid);
        // B is loaded right behind A: their entries arrive in one trip
        bool validB = false;
        uint4 eB = make_uint4(0, 0, kDeadMeta, 0);
        const bool haveB = next.peek(eB, validB);
        issue_fence();
        ACL_MARK(wo, PH_ENTRIES);
        struct LaneOp {  // the lane's one remaining op + what its tasks need to know about the child state
            uint32_t flags, dlevel, base, nrows, Kk, key, maxd;  // Kk = K | k << 16
            uint32_t cbase, cnrows, ckey;                        // child's hashed probe (cnrows == 0: the child is not "one hashed probe")
            uint32_t cdl, cmaxd;                                 // ... its dispatch-depth offset and the child program's deepest inlined state
        };
        auto lane_op = [&](uint32_t m, LaneOp &L) -> bool {  // false: not a simple parent
            if (m == kDeadMeta || !(m & kProbedBit) || meta_key(m) < g.nslots) return false;
            const SlotProg sp = progs[meta_slot(m)];
            if (sp.n_main != sp.n_probe + 1 || (CMB && sp.combine)) return false;
            const FwdOp o = ops[sp.first + sp.n_probe];
            if (!(o.flags & OP_ENUM) || (o.flags & (OP_PUSH_SAME | OP_REFLEX | OP_PROBE_HASH))) return false;
            L.flags = o.flags; L.dlevel = o.dlevel; L.base = o.base; L.nrows = o.nrows; L.Kk = o.K | (o.k << 16); L.key = o.key; L.maxd = sp.max_dlevel;
            const SlotProg cp = progs[o.key];
            L.cbase = 0; L.cnrows = 0; L.ckey = 0; L.cdl = 0; L.cmaxd = cp.max_dlevel;
            if (cp.n_probe == 1) {
                const FwdOp co = ops[cp.first];
                if (co.flags == OP_PROBE_HASH) { L.cbase = co.base; L.cnrows = co.nrows; L.ckey = co.key; L.cdl = co.dlevel; }
            }
            return true;
        };
        const uint32_t m0 = (uint32_t)__builtin_amdgcn_readlane((int)meta, (int)(__ffsll((unsigned long long)vb) - 1));
        LaneOp LA{}, LB{};
        bool simple;
        const uint64_t vbB = haveB ? __ballot(validB) : 0ull;
        // (same slot, level, key: the deep levels.  States of the two-hop slot may differ in their LEVEL: with two-hop rows one iteration holds that slot's states
        //  of two adjacent levels side by side -- children of one-hop rows and grandchildren of two-hop ones.  Nothing a segment of one slot relies on below
        //  depends on the level: lane_op() does not look at it, seg_tasks() takes each lane's own, the direct form keeps it per task.)
        const uint32_t lvbits = (E8 && meta_slot(m0) == g.hop2_slot) ? (63u << 13) : 0u;  // (uniform; hop2_slot names no slot while the rows are not in use)
        const bool oneslot = !__ballot(valid && ((meta ^ m0) & ~lvbits) != 0u) && !(vbB && __ballot(validB && ((eB.z ^ m0) & ~lvbits) != 0u));
        if (oneslot) {
            // ---- the deep levels' shape, without the task list's round trips (round 5): ONE slot, level and subject key for both segments, children
            // that are "one hashed probe + authoritative leaf flags" (what flush_simple takes).  Decided and run HERE, while the program's fields are
            // still scalars.  The lane that creates a task already holds its degree, so the prefix sums run over the creating lanes' registers
            // (compaction keeps the order: the prefix over lanes IS the prefix over tasks), each lane writes its task with the edge base already
            // rebased and sets its head bit itself, and every child carries the same meta: no count / meta / subject-id stores, no read-back of the
            // counts, no read-modify-write of the edge bases -- the prologue's chain of dependent LDS trips (14 % of the walk's wave-time,
            // profiles/r05_ab_split_units.txt) shrinks to one fence.
            // HOP (states of the two-hop slot while two-hop rows are in use; uniform, decided per pair): the same form reading the two-hop rows and carrying the
            // children's level per task.  Instantiated apart, so that every other pair runs the instructions it always ran.  true: the pair is done.
            auto direct = [&](auto hop_tag) -> bool {
                constexpr bool HOP = decltype(hop_tag)::value;
                LaneOp LD{};  // (a copy of its own: nothing of it is live behind this block, so the general path's LA / LB are not carried -- spilled -- across it)
                if (!lane_op(m0, LD)) return false;
                // (the program's fields come out of the LDS copy in VGPRs, uniform or not: pinned into SGPRs here -- a dozen VGPRs held across the
                //  gathers otherwise, and the walk has none to spare: 6 waves per SIMD allow 80, it took 72 when round 5 chose that shape
                //  (profiles/r05_ab_block_shape.txt) and takes nearly all of them now (tools/resusage.py))
                uint32_t lv = meta_level(m0);
                if (HOP && (__ballot(valid && meta != m0) || (vbB && __ballot(validB && eB.z != m0))))  // levels differ: the depth guards take the pair's highest
                    lv = wave_max(max(valid ? meta_level(meta) : 0u, (vbB && validB) ? meta_level(eB.z) : 0u));
                const uint32_t Lv = lv + uniform(LD.dlevel);
                const uint32_t d_cnrows = uniform(LD.cnrows), d_cbase = uniform(LD.cbase), d_base = uniform(LD.base), d_nrows = uniform(LD.nrows), d_Kk = uniform(LD.Kk), d_key = uniform(LD.key);
                if (!(d_cnrows != 0u && uniform(LD.ckey) == meta_key(m0) && (uniform(LD.flags) & OP_LEAFBIT) != 0u && Lv + 1u <= kMaxLevels && Lv + 1u + uniform(LD.cdl) <= kMaxLevels &&
                      Lv + 1u + uniform(LD.cmaxd) <= kMaxLevels && lv + uniform(LD.maxd) <= kMaxLevels))
                    return false;
                const bool dpair = vbB != 0;
                if (dpair) next.take();
                const uint2 *__restrict__ dmeta2 = reinterpret_cast<const uint2 *>(g.meta);
                const uint32_t rK = d_Kk & 0xFFFFu, rk = d_Kk >> 16;
                const bool vB = dpair && validB;
                // Two-hop rows (plan.hpp Snapshot::hop2_*): the row of a state of the self-nested class holds its children (probed, not pushed) AND their children
                // (probed and pushed, one level further on) -- two of three states of the class are never written, read back, gathered or scheduled.  Taken
                // where the depth guards hold for BOTH hops (the four conditions above, once more for a state one level further on); at the depth limit the
                // pair runs on the one-hop rows exactly as it always did.  (uniform)
                bool h2 = HOP && d_key == g.hop2_slot && d_nrows == g.hop2_nrows && Lv + 2u + uniform(LD.dlevel) <= kMaxLevels &&
                          Lv + 2u + uniform(LD.dlevel) + uniform(LD.cdl) <= kMaxLevels && Lv + 2u + uniform(LD.dlevel) + uniform(LD.cmaxd) <= kMaxLevels &&
                          Lv + 1u + uniform(LD.maxd) <= kMaxLevels;
                const uint32_t gbase = h2 ? g.hop2_base : d_base, gK = h2 ? 1u : rK, gk = h2 ? 0u : rk;
                // all six gathers in flight together
                const uint32_t hvA = ans_get<true>(has, valid ? req : wo.first, wo.first), hvB = ans_get<true>(has, vB ? eB.y : wo.first, wo.first);
                const bool inA = valid && id < d_nrows, inB = vB && eB.x < d_nrows;
                uint2 mdA = gld(dmeta2, gbase + (inA ? id * gK + gk : 0u)), mdB = gld(dmeta2, gbase + (inB ? eB.x * gK + gk : 0u));
                // the subject's row of the child's probe is a constant of the REQUEST: for the snapshot's hot hashed class (DevGraph::hot_*) every
                // request's descriptor was fetched once, when the unit was seeded (s_sd) -- two LDS reads here, not two gathers per pair of segments
                const bool hotd = d_cbase == g.hot_cbase && d_cnrows == g.hot_cnrows && uniform(LD.ckey) == g.hot_ckey;  // (uniform)
                const bool okA = valid && e.w < d_cnrows, okB = vB && eB.w < d_cnrows;
                uint2 sdA, sdB;
                if (hotd) {
                    sdA = wo.ssd[valid ? req - wo.first : 0u];
                    sdB = wo.ssd[vB ? eB.y - wo.first : 0u];
                } else {
                    sdA = gld(dmeta2, d_cbase + (okA ? e.w : 0u));
                    sdB = gld(dmeta2, d_cbase + (okB ? eB.w : 0u));
                }
                issue_fence();
                ACL_MARK(wo, PH_GATHERS);
                if (!hotd) {
                    if (!(okA && sdA.y != 0u)) sdA = make_uint2(0u, 1u);  // no row: the reserved empty bucket (what s_sd holds for such a request)
                    if (!(okB && sdB.y != 0u)) sdB = make_uint2(0u, 1u);
                }
                uint32_t degA = (valid && !hvA && inA && mdA.y > mdA.x) ? mdA.y - mdA.x : 0u;
                uint32_t degB = (vB && !hvB && inB && mdB.y > mdB.x) ? mdB.y - mdB.x : 0u;
                uint32_t inclA = wave_incl_scan(degA, lane), totA = wave_last(inclA);
                uint32_t inclB = wave_incl_scan(degB, lane) + totA, total = wave_last(inclB);
                if (HOP && h2 && total > 64u * kHeadWords) {
                    // (rare: a pair of two-hop rows alone always fits the window -- kHop2MaxRow -- so this pair mixes them with long one-hop rows.  Expanded
                    //  again from the one-hop descriptors: a second descriptor trip; only what overflows there too is an overflow of the form)
                    h2 = false;
                    mdA = gld(dmeta2, d_base + (inA ? id * rK + rk : 0u));
                    mdB = gld(dmeta2, d_base + (inB ? eB.x * rK + rk : 0u));
                    issue_fence();
                    degA = (valid && !hvA && inA && mdA.y > mdA.x) ? mdA.y - mdA.x : 0u;
                    degB = (vB && !hvB && inB && mdB.y > mdB.x) ? mdB.y - mdB.x : 0u;
                    inclA = wave_incl_scan(degA, lane);
                    inclB = wave_incl_scan(degB, lane) + wave_last(inclA);
                    total = wave_last(inclB);
                }
#if ACL_PROFILE_PHASES  // (instrumented builds: pairs of the two-hop slot expanded from two-hop rows, and those that fell back to the one-hop rows -- depth or window)
                if (HOP && lane == 0) wo.cold->prof[h2 ? 18 : 19] += 1u;
#endif
                if (total > 64u * kHeadWords || __ballot(degA > kMaxRow || degB > kMaxRow)) {
                    // more children than the head-bit window maps (an average fan-out beyond 16), or a row beyond the enumeration limit: this form has
                    // no second round (one would have to keep the pair's registers across the steps, and the walk's VGPR budget is used up -- see above).  The batch is
                    // redone on the level loop and the host switches the form off for this snapshot (kOverflowDirect; a row beyond kMaxRow fails
                    // the call as it does on every path).
                    if (lane == 0) *wo.cold->overflow = __ballot(degA > kMaxRow || degB > kMaxRow) ? 2u : kOverflowDirect;
                    wo.cur = kNoSpace;
                    return true;
                }
                if (!total) return true;
                const uint64_t bA = __ballot(degA != 0u), bB = __ballot(degB != 0u);
                const uint32_t cladd = (uniform(LD.dlevel) + 1u) << 13;  // (HOP: a task carries its children's level -- the parent's own + the op's offset + 1)
                if (degA) {
                    const uint32_t ex = inclA - degA;
                    t.a[lanes_below(bA)] = make_uint4(mdA.x - ex, sdA.x, sdA.y, HOP ? ((req - wo.first) << 19) | ((meta & (63u << 13)) + cladd) : req - wo.first);
                    atomicOr(reinterpret_cast<unsigned long long *>(&t.heads[ex >> 6]), 1ull << (ex & 63u));
                }
                if (degB) {
                    const uint32_t ex = inclB - degB;
                    t.a[(uint32_t)__popcll(bA) + lanes_below(bB)] = make_uint4(mdB.x - ex, sdB.x, sdB.y, HOP ? ((eB.y - wo.first) << 19) | ((eB.z & (63u << 13)) + cladd) : eB.y - wo.first);
                    atomicOr(reinterpret_cast<unsigned long long *>(&t.heads[ex >> 6]), 1ull << (ex & 63u));
                }
                wave_lds_fence();
                ACL_MARK(wo, PH_TASKS);
                if (HOP)
                    simple_steps<LOCAL, true, true, true>(t, total, wo, lane, g.edges, reinterpret_cast<const uint4 *>(g.buckets), has, err, d_key, h2 ? (1u << 13) : 0u);
                else
                    simple_steps<LOCAL, true, true>(t, total, wo, lane, g.edges, reinterpret_cast<const uint4 *>(g.buckets), has, err, make_meta(d_key, Lv + 1u, meta_key(m0)));
                if (lane < kHeadWords) t.heads[lane] = 0ull;
                wave_lds_fence();
                ACL_MARK(wo, PH_PUSH);
                return true;
            };
            if constexpr (E8) {
                if (!(g.walk_flags & kWalkNoDirect) && (__builtin_expect(lvbits != 0u, 0) ? direct(std::true_type{}) : direct(std::false_type{}))) return;
            }
            simple = lane_op(m0, LA);  // wave-uniform argument
            LB = LA;
        } else {
            simple = !__ballot(valid && !lane_op(meta, LA));
        }
        if (simple) {
            bool pairB = vbB != 0;
            if (pairB && !oneslot) pairB = !__ballot(validB && !lane_op(eB.z, LB));
            if (pairB) next.take();
            else validB = false;
            const uint2 *__restrict__ meta2 = reinterpret_cast<const uint2 *>(g.meta);
            // (the subject's row descriptor is gathered here: reading the unit's LDS copy, s_sd, as the direct form does took the walk past its 80 VGPRs -- 30 to 63 spilled)
            auto subj_desc = [&](const uint4 &se, bool sv, const LaneOp &L) -> uint2 {
                const bool ok = sv && meta_key(se.z) == L.ckey && se.w < L.cnrows;
                const uint2 d = gld(meta2, L.cbase + (ok ? se.w : 0u));
                return (ok && d.y != 0u) ? d : make_uint2(0u, 1u);  // {first bucket, the row's y}; no row: the reserved empty bucket
            };
            auto row_desc = [&](uint32_t rid, bool in, const LaneOp &L) -> uint2 { return gld(meta2, L.base + (in ? rid * (L.Kk & 0xFFFFu) + (L.Kk >> 16) : 0u)); };
            // tasks of one simple segment -> LDS task slots [Tb, Tb + n); returns n
            auto seg_tasks = [&](const uint4 &se, bool sv, uint32_t hv, uint2 md, uint2 sd, bool inrow, const LaneOp &L, uint32_t Tb) -> uint32_t {
                const bool act = sv && !hv;
                const uint32_t lv = meta_level(se.z), Lv = lv + L.dlevel;
                bool derr = act && lv + L.maxd > kMaxLevels, want = false;
                if (act && Lv <= kMaxLevels && inrow && md.y > md.x) {
                    if (Lv + 1 > kMaxLevels) derr = true;
                    else if (md.y - md.x > kMaxRow) *wo.cold->overflow = 2u;
                    else want = true;
                }
                if (derr) ans_set<E8>(err, se.y, wo.first, ITEM_ERR_DEPTH);
                const uint64_t b = __ballot(want);
                if (want) {
                    const uint32_t q = Tb + lanes_below(b);
                    t.a[q] = make_uint4(md.x, sd.x, sd.y, se.y);
                    t.count[q] = (md.y - md.x) | ((L.flags & OP_LEAFBIT) ? kLeafAuthBit : 0u);
                    t.meta[q] = make_meta(L.key, Lv + 1, meta_key(se.z));
                    t.sid[q] = se.w;
                }
                return (uint32_t)__popcll(b);
            };
            // all six gathers in flight together
            const uint32_t hvA = ans_get<E8>(has, valid ? req : (E8 ? wo.first : 0u), wo.first);
            const bool inA = valid && id < LA.nrows;
            const uint2 mdA = row_desc(id, inA, LA);
            const uint2 sdA = subj_desc(e, valid, LA);
            uint32_t hvB = 0;
            uint2 mdB = make_uint2(0, 0), sdB = make_uint2(0, 1);
            const bool inB = validB && eB.x < LB.nrows;
            if (pairB) {
                hvB = ans_get<E8>(has, validB ? eB.y : (E8 ? wo.first : 0u), wo.first);
                mdB = row_desc(eB.x, inB, LB);
                sdB = subj_desc(eB, validB, LB);
            }
            issue_fence();
            ACL_MARK(wo, PH_GATHERS);
#if ACL_PROFILE_PHASES  // (instrumented builds: entries the deep levels read, and how many of them belong to requests that were answered meanwhile)
            {
                const uint32_t nA = (uint32_t)__popcll(__ballot(valid)), dA = (uint32_t)__popcll(__ballot(valid && hvA != 0u));
                const uint32_t nB = pairB ? (uint32_t)__popcll(__ballot(validB)) : 0u, dB = pairB ? (uint32_t)__popcll(__ballot(validB && hvB != 0u)) : 0u;
                if (lane == 0) {
                    wo.cold->prof[12] += nA + nB;
                    wo.cold->prof[13] += dA + dB;
                    wo.cold->prof[14] += 1u + (pairB ? 1u : 0u);                                  // segments walked
                    wo.cold->prof[15] += (nA + nB - dA - dB <= 64u && pairB) ? 1u : 0u;            // pairs whose live entries would fit ONE segment
                }
            }
#endif
            uint32_t T = seg_tasks(e, valid, hvA, mdA, sdA, inA, LA, 0u);
            if (pairB) T += seg_tasks(eB, validB, hvB, mdB, sdB, inB, LB, T);
            ACL_MARK(wo, PH_TASKS);
            if (T) flush_tasks<true, SHARDED, LOCAL, true, CMB>(t, T, wo, lane, g, progs, ops, g.edges, has, err, sh, oneslot);
            ACL_MARK(wo, PH_PUSH);
            return;
        }
    }
    // ---- generic path: interpret the state's program.  Tasks are only RECORDED while the ops run (one segment of the LDS
    // list per enumerating op) and expanded afterwards, segment by segment, when the interpreter's per-lane state is dead:
    // the expansions (flush_simple / flush_probes) are the register-hungry part and no longer stack on top of it.
    // (Per-op segments keep the tasks of one flush uniform in child slot, which is what the fast paths need.)
    constexpr uint32_t kMaxSeg = 4;
    uint4 ee = e;
    uint32_t jstart = 0;
    bool hit = false;
    uint32_t cbase = 0;  // CMB: first leaf cell of this lane's combine state (allocated on the first pass over the entry)
    for (;;) {
        // (re)derive everything from the entry: nothing but `ee`, `hit` and `jstart` lives across the expansions below
        asm volatile("" : "+v"(ee.x), "+v"(ee.y), "+v"(ee.z), "+v"(ee.w));
        const uint32_t id = ee.x, req = ee.y, meta = ee.z, sid = ee.w;
        bool active = valid && meta != kDeadMeta;
        if (active && (hit || ans_get<E8>(has, req, wo.first))) active = false;  // request already answered HAS: drop its pending work
        const uint32_t slot = meta_slot(meta), level = meta_level(meta), key = meta_key(meta);
        const bool probed = meta & kProbedBit;  // the parent already ran this state's probes
        SlotProg p{};
        if (active) p = progs[slot];
        bool cmb = false;
        if (CMB) {
            cmb = active && p.combine != 0;
            if (jstart == 0) {  // first pass over the entry: leaf cells, the node, the leaves' depth errors
                bool over = false;
                if (cmb) {
                    const uint32_t c0 = atomicAdd(co.ncell, p.nleaves), ni = atomicAdd(co.nnode, 1u);
                    over = c0 + p.nleaves > co.cell_cap || ni >= co.node_cap;
                    if (!over) {
                        cbase = co.cell0 + c0;
                        for (uint32_t k = 0; k < p.nleaves; k++) {
                            has[cbase + k] = 0;
                            err[cbase + k] = ITEM_ERR_NONE;
                        }
                        co.nodes[ni] = make_uint4(req, cbase, slot | (co.iter << 16), 0u);
                    }
                }
                if (__ballot(over)) {  // out of cells / nodes: the pass is redone elsewhere (single launch -> level loop) or fails (level loop)
                    if (LOCAL) {
                        if (lane == 0) *wo.cold->overflow = 1u;
                        wo.cur = kNoSpace;
                    } else if (lane == 0) {
                        *wo.cold->overflow = SHARDED ? kOverflowPools : 3u;
                    }
                    if (over) active = cmb = false;
                }
                // (the zeroes above are acknowledged before any hit is stored into a cell, by this lane or by the lanes that expand its tasks)
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                if (cmb) {
                    const uint32_t *be = co.bexpr + p.combine + 1;  // deepest inlined dispatch offset per leaf (0 = the direct ops)
                    for (uint32_t k = 0; k <= p.nleaves; k++)
                        if (level + be[k] > kMaxLevels) err[k ? cbase + k - 1u : req] = ITEM_ERR_DEPTH;
                }
            }
        }
        const uint32_t j0 = probed ? p.n_probe : 0u;
        const uint32_t j1 = active ? ((probed || key >= g.nslots) ? p.n_main : p.n_total) : 0u;
        bool depth_err = active && !cmb && level + p.max_dlevel > kMaxLevels;
        uint32_t T = 0, nseg = 0, seg_end[kMaxSeg] = {0, 0, 0, 0};
            const uint32_t maxops = uniform(wave_max(j1 > j0 ? j1 - j0 : 0u));
        uint32_t jj = jstart;
        for (; jj < maxops; jj++) {
            const uint32_t j = j0 + jj;
            bool want = false;
            uint32_t tstart = 0, tcount = 0, tmeta = 0, tcell = req;
            if (j < j1) {
                const FwdOp op = ops[p.first + j];
                const uint32_t L = level + op.dlevel;
                const bool leafop = CMB && op.leaf != 0;  // the op answers one of the state's leaf cells, not the entry's own cell
                if (leafop) tcell = cbase + op.leaf - 1u;
                if (L <= kMaxLevels) {
                    bool h = false, derr = false;  // this op's probe hit / it would dispatch beyond the depth limit
                    if (op.flags & OP_REFLEX) {
                        h = key == op.key && id == sid;
                    } else if (op.flags & OP_PUSH_SAME) {
                        if (L + 1 > kMaxLevels) derr = true;
                        else {
                            want = true;
                            tstart = id;
                            tcount = 1u | kSelfBit;
                            tmeta = make_meta(op.key, L + 1, key);
                        }
                    } else if (op.flags & OP_PROBE_HASH) {
                        if (key == op.key) h = subject_row_contains(g, op, id, sid);
                    } else if (id < op.nrows) {
                        const uint2 md = row_meta(g, op, id);
                        if (md.y > md.x) {
                            if ((op.flags & OP_PROBE) && key == op.key) h = row_contains(g.edges, md.x, md.y, sid);
                            if (op.flags & OP_ENUM) {
                                if (L + 1 > kMaxLevels) derr = true;
                                else if (md.y - md.x > kMaxRow) *wo.cold->overflow = 2u;
                                else if (!(leafop ? h : (hit || h))) {
                                    want = true;
                                    tstart = md.x;
                                    tcount = (md.y - md.x) | ((op.flags & OP_LEAFBIT) ? kLeafAuthBit : 0u) | ((CMB && (op.flags & OP_ALL)) ? kAllBit : 0u);
                                    tmeta = make_meta(op.key, L + 1, key);
                                }
                            }
                        }
                    }
                    if (leafop) {
                        if (h) has[tcell] = 1;
                        else if (derr) err[tcell] = ITEM_ERR_DEPTH;
                    } else {
                        hit |= h;
                        depth_err |= derr;
                    }
                }
            }
            const uint64_t b = __ballot(want);
            if (b) {
                if (want) {
                    const uint32_t q = T + lanes_below(b);
                    t.a[q] = make_uint4(tstart, 0u, 1u, tcell);  // (the subject's row is looked up by the expansion that needs it)
                    t.count[q] = tcount;
                    t.meta[q] = tmeta;
                    t.sid[q] = sid;
                }
                T += (uint32_t)__popcll(b);
                seg_end[nseg++] = T;
                if (nseg == kMaxSeg || T > kTaskCap - 64) {  // list (nearly) full: expand what is recorded, then resume with the next op
                    jj++;
                    break;
                }
            }
        }
        jstart = jj;
        if (active) {
            if (hit) ans_set<E8>(has, req, wo.first, 1);
            else if (depth_err) ans_set<E8>(err, req, wo.first, ITEM_ERR_DEPTH);
        }
        const bool more = jstart < maxops;
        // ---- expand the recorded segments (the interpreter's state is dead from here to the loop's top)
        uint32_t a = 0;
#pragma unroll 1
        for (uint32_t k = 0; k < nseg; k++) {
            const uint32_t bnd = seg_end[k], cnt = bnd - a;  // cnt <= 64
            if (a) {  // bring the segment to the front of the list (expansions address tasks from 0)
                uint4 c0 = make_uint4(0, 0, 0, 0);
                uint32_t c1 = 0, c3 = 0, c4 = 0;
                if (lane < cnt) { c0 = t.a[a + lane]; c1 = t.count[a + lane]; c3 = t.meta[a + lane]; c4 = t.sid[a + lane]; }
                wave_lds_fence();
                if (lane < cnt) { t.a[lane] = c0; t.count[lane] = c1; t.meta[lane] = c3; t.sid[lane] = c4; }
            }
            flush_tasks<true, SHARDED, LOCAL, false, CMB>(t, cnt, wo, lane, g, progs, ops, g.edges, has, err, sh, false, co);
            a = bnd;
        }
        if (!more) break;
    }
    ACL_MARK(wo, PH_GENERIC);
}

// the program table (a few hundred bytes for real schemas) is copied into LDS when it fits
template <bool LDSPROG>
__device__ __forceinline__ void load_programs(const DevGraph &g, uint4 *s_prog, const SlotProg *&progs, const FwdOp *&ops, uint32_t nthreads) {
    progs = g.progs;
    ops = g.ops;
    if (LDSPROG) {
        const uint32_t np = g.nslots * 2, no = g.nops * 2;
        for (uint32_t i = threadIdx.x; i < np; i += nthreads) s_prog[i] = reinterpret_cast<const uint4 *>(g.progs)[i];
        for (uint32_t i = threadIdx.x; i < no; i += nthreads) s_prog[np + i] = reinterpret_cast<const uint4 *>(g.ops)[i];
        __syncthreads();
        progs = reinterpret_cast<const SlotProg *>(s_prog);
        ops = reinterpret_cast<const FwdOp *>(s_prog + np);
    }
}

__device__ __forceinline__ WaveOut chunked_out(const DevFrontier &f, uint32_t iter, uint32_t wave, WaveOutCold *cold, uint32_t lane) {
    if (lane == 0) {
        cold->counts = f.counts[iter & 1u];
        cold->nchunks = f.nchunks + iter;
        cold->overflow = f.overflow;
        cold->nwaves = f.nwaves;
        cold->max_chunks = f.max_chunks;
        cold->cap = 0;
    }
    wave_lds_fence();
    WaveOut wo;
    wo.buf = f.buf[iter & 1u];
    wo.cur = wave;
    wo.fill = 0;
    wo.produced = 0;
    wo.cold = cold;
    wo.lcap = 0;
    return wo;
}

// Segment-major walk over the chunks iteration `iter - 1` produced.  Chunks are mostly part-filled, so their low segments
// carry the work; walking all chunks' segment 0 first, then segment 1, ... spreads it evenly over the waves (each segment
// layer is rotated so that one wave does not keep landing on the same chunk).  The fill counts of the wave's next 64
// segment slots are fetched by its 64 lanes in ONE gather; the loop then reads them with readlane -- not one dependent
// load per slot (most slots are empty: 16+ per wave and level).
struct ChunkWalk {
    const uint4 *__restrict__ in;
    uint32_t lane;
    const uint32_t *slots;  // LDS, wave-private, of the wave's next 64 segment slots: [0, 64) first entry of the segment (chunk * kChunk + segment * 64),
                            // [64, 128) entries the chunk holds from that segment on -- in LDS, not in two VGPRs that live across every expansion
    uint64_t work;
    __device__ __forceinline__ void load(int wl, uint4 &e, bool &valid) const {
        const uint32_t at = uniform(slots[wl]), left = uniform(slots[64 + wl]);  // left >= 1: the slot's work bit is set
        valid = lane < left;
        e = gld(in, at + (valid ? lane : 0u));  // unconditional (a load under `if` is waited for where the branch rejoins); the caller masks by `valid`
    }
    __device__ __forceinline__ bool peek(uint4 &e, bool &valid) const {
        if (!work) return false;
        load(__ffsll((unsigned long long)work) - 1, e, valid);
        return true;
    }
    __device__ __forceinline__ void take() { work &= work - 1; }
};

template <bool LDSPROG, bool SHARDED, bool CMB = false>
__global__ __launch_bounds__(kBlock, ACL_MIN_WAVES_PER_SIMD) void k_expand(DevGraph g, DevFrontier f, uint32_t iter, uint8_t *has, uint8_t *err,
                                                                           DevShard sh) {
    __shared__ TaskLds lds[kWavesPerBlock];
    __shared__ WaveOutCold s_cold[kWavesPerBlock];
    __shared__ uint32_t s_slots[kWavesPerBlock][128];
    extern __shared__ uint4 s_prog[];  // dynamic: sized by the launcher to THIS snapshot's program table (a fixed 8 KiB cost two blocks per CU)
    const SlotProg *progs;
    const FwdOp *ops;
    load_programs<LDSPROG>(g, s_prog, progs, ops, kBlock);
    const uint32_t lane = lane_id();
    const uint32_t wib = uniform(threadIdx.x >> 6);  // (wave-uniform, and the compiler is told so: per-wave pointers then live in SGPRs)
    TaskLds &t = lds[wib];
    if (lane < kHeadWords) t.heads[lane] = 0ull;  // (flush_simple's head bits: zero between expansions)
    const uint32_t wave = blockIdx.x * kWavesPerBlock + wib, nwaves = f.nwaves;
    const uint32_t pin = (iter + 1) & 1u;  // iteration i reads parity (i-1)&1
    const uint32_t *__restrict__ in_counts = f.counts[pin];
    const bool live = !*f.overflow && f.any[iter - 1];
    const uint32_t C = live ? nwaves + min(f.nchunks[iter - 1], f.max_chunks - nwaves) : 0u;
    WaveOut wo = chunked_out(f, iter, wave, &s_cold[wib], lane);
    uint32_t *slots = s_slots[wib];
    ChunkWalk cw{f.buf[pin], lane, slots, 0ull};
    CombineOut co;
    if (CMB) co = CombineOut{g.nodes, g.ccount + 1, g.ccount, g.node_cap, g.cell_cap, g.cell0, iter, g.bexpr};
    const uint32_t nslot = C * kSegsPerChunk;
    for (uint32_t x0 = wave; x0 < nslot; x0 += 64 * nwaves) {
        // (once per 64 slots: keep the division's precomputed reciprocal out of a VGPR that would live across every expansion)
        uint32_t Cl = C;
        asm volatile("" : "+s"(Cl));
        const uint32_t xl = x0 + lane * nwaves;
        uint32_t lat = 0, lcnt = 0;
        if (xl < nslot) {
            const uint32_t ls = xl / Cl, lc = (xl % Cl + ls * 509u) % Cl;
            lcnt = in_counts[lc];
            lcnt = lcnt > ls * 64 ? lcnt - ls * 64 : 0u;  // entries of this slot's segment and beyond
            lat = lc * kChunk + ls * 64;
        }
        wave_lds_fence();  // (the previous round's readers are done)
        slots[lane] = lat;
        slots[64 + lane] = lcnt;
        cw.work = __ballot(lcnt != 0);
        wave_lds_fence();
        while (cw.work) {
            const int wl = __ffsll((unsigned long long)cw.work) - 1;
            cw.work &= cw.work - 1;
            uint4 e;
            bool valid;
            cw.load(wl, e, valid);
            process_segment<SHARDED, false, CMB>(e, valid, cw, t, wo, lane, g, progs, ops, has, err, sh, co);
        }
    }
    if (lane == 0) {
        if (wo.cur != kNoSpace) wo.cold->counts[wo.cur] = wo.fill;  // also publishes 0 for an unused static chunk
        if (wo.produced) f.any[iter] = 1u;
    }
}

// ------------------------------------------------------------ single launch
// Small batches -- the proxy's own call shape: one item per check expression (reference pkg/authz/check.go:76-94), one per
// watch update (watch.go:50), a few thousand after micro-batching.  The level-synchronous path costs a launch (and part of
// a host round trip) per dispatch level, ~17 us each whatever the batch size; here ONE launch answers the batch: every wave
// takes `rpw` requests, seeds them in registers, and walks them through all levels itself with a wave-private frontier
// (two regions of the frontier buffers, ping-pong), then writes the answers (k_seed + k_expand x levels + k_finalize fused).
// No wave ever reads another wave's entries, so there is no grid barrier and no inter-level visibility to arrange beyond
// the wave's own release/acquire.  A wave that outgrows its region raises `overflow`; the host redoes the batch on the
// level-synchronous path.  Same segment processor, same decisions.
template <bool E8>
struct LocalWalk {
    const uint4 *__restrict__ in;  // (E8: 8-byte entries, see put_entry)
    uint32_t n, s, lane;  // entries in the input region; the segment being processed (segments are claimed in pairs: s even)
    bool second;          // the pair's second segment is still to be taken
    const uint2 *sreq;    // E8: the unit's per-request constants {subject id, subject key} (LDS)
    uint32_t first;       // E8: the unit's first request
    uint2 rawB = make_uint2(0u, 0u);  // the pair's second segment, fetched (undecoded) when the pair was claimed (k_check_local's claim loop)
    bool have_rawB = false;
    __device__ __forceinline__ uint2 raw(uint32_t i) const { return gld(reinterpret_cast<const uint2 *>(in), i); }
    __device__ __forceinline__ uint4 at(uint32_t i) const {
        if (E8) return decode_entry8(raw(i), sreq, first);
        return gld(in, i);
    }
    __device__ __forceinline__ bool peek(uint4 &e, bool &valid) const {
        if (!second || (s + 1) * 64 >= n) return false;
        valid = (s + 1) * 64 + lane < n;
        if (E8 && have_rawB) e = decode_entry8(rawB, sreq, first);
        else e = at(valid ? (s + 1) * 64 + lane : (s + 1) * 64);  // unconditional, like ChunkWalk::load
        return true;
    }
    __device__ __forceinline__ void take() { second = false; }
};
struct NoNext {
    __device__ __forceinline__ bool peek(uint4 &, bool &) const { return false; }
    __device__ __forceinline__ void take() {}
};

// Work = units of `rpw` (<= 256) consecutive requests, one unit per BLOCK at a time (block b takes units b, b + nblocks, ...).
// The block's four waves walk the unit together, level by level, inside the block's private frontier region: a level's
// segments are claimed pair by pair through an LDS counter, children are appended through an LDS cursor, and one block
// barrier separates the levels.  Sharing a unit between four waves is what keeps the launch's tail short: requests differ
// 100-fold in work (a first-level hit against a full five-level miss), and a wave that walked its own 43 requests alone
// finished anywhere between 0.5x and 1.6x the mean -- a third of the wave-time was idle waiting for the slowest
// (profiles/r02_pmc_walk.txt); a unit of 4 x 43 requests varies half as much, and inside it the work is shared per level.
// Block b starts on unit b; further units (batches beyond 256 requests per resident block) are handed out through
// `next_unit`, one atomic per BLOCK-unit -- per wave-unit the same counter cost ~12 ns per unit in same-address contention
// (profiles/r02_walk_units_per_wave.txt).
struct InlineItems {  // up to four 16-byte items passed by value (kernel arguments)
    uint4 v[4];
};
#ifndef ACL_LOCAL_WAVES_PER_SIMD
#define ACL_LOCAL_WAVES_PER_SIMD 6  // (round 5; 8 in rounds 2-4: see ACL_LOCAL_WIDE)
#endif
// Waves per block = waves that share one unit.  Two instantiations: kLocalNarrow for batches that do not fill the chip (a unit is a handful of
// requests: more, smaller blocks) and kLocalWide for chip-filling ones -- requests differ 100-fold in work, so the more requests (and waves) a
// unit pools, the less the slowest block's sum sticks out: C4's 262 144-item batch 303 us with 4 waves per block (2 048 units of 128 requests),
// 286 us with 8, 276 us with 16 (512 units of 512), same-box A/B in profiles/r03_waves_per_block_ab.txt.
#ifndef ACL_LOCAL_WIDE
#define ACL_LOCAL_WIDE 12  // Round 5: 12 waves per block, two blocks per CU = 6 waves per SIMD with 72 VGPRs and three children per lane and step -- C4 221.4 -> 216.8 us, the
                           // 100 M-relationship replica 294.4 -> 283.8 us (16 waves at 64 VGPRs and two children per step until then: every attempt to add live state to
                           // the fast paths at 64 VGPRs ended in spills; 12 waves had lost to 16 in round 4, when a child still cost two bucket gathers = 8 VGPRs more).
                           // 14 waves: 275 us, 10 waves x 3 blocks: 226 us, four children per step: 227 us (profiles/r05_ab_block_shape.txt)
#endif
constexpr int kLocalNarrow = 4, kLocalWide = ACL_LOCAL_WIDE;
template <bool LDSPROG, int WAVES, bool CMB = false>
__global__ __launch_bounds__(WAVES * 64, ACL_LOCAL_WAVES_PER_SIMD) void k_check_local(DevGraph g, const uint4 *__restrict__ items, uint32_t n, uint32_t rpw,
                                                                                  uint32_t nunits, uint32_t nstatic, uint32_t rdyn, uint32_t *next_unit, uint4 *buf0, uint4 *buf1,
                                                                                  uint32_t cap,
                                                                                  uint32_t *overflow, uint8_t *has, uint8_t *err, uint8_t *perm_out,
                                                                                  int32_t *err_out, uint32_t *max_level, uint32_t skew, uint32_t *done_ctr, uint32_t *done_flag,
                                                                                  uint32_t done_val, InlineItems inl) {
    __shared__ TaskLds lds[WAVES];
    __shared__ WaveOutCold s_cold[WAVES];
    // output cursor / segment-claim counter of level L live in slot L % 3: written during L, read at the start of L + 1, cleared at the
    // start of L + 2 (every wave has read them by then) and reused at L + 3 -- ONE block barrier per level instead of three.
    // (Two half-units whose levels turn over independently, without the barrier, won on C4 and lost on the 100 M-relationship replica:
    //  profiles/r05_ab_split_units.txt.)
    // (s_cursors: one array -- the per-unit reset is ONE store through one address, two arrays cost a spilled VGPR.  Six words are used; the seventh
    //  is spare, and dropping it moves the LDS layout and with it the register allocation: to be done with a measurement, not in passing.)
    constexpr uint32_t kCursorWords = 7;
    __shared__ uint32_t s_cursors[kCursorWords], s_stop, s_unit;
    uint32_t *const s_fill = s_cursors, *const s_next = s_cursors + 3;
    __shared__ uint32_t s_ccount[2];  // CMB: {leaf cells, nodes} of the unit being walked
    constexpr bool E8 = !CMB;  // 8-byte frontier entries (put_entry)
    __shared__ uint2 s_req[E8 ? WAVES * 64 : 1];  // E8: {subject id, subject key} of the unit's requests
    // E8: {first bucket, the row's y} of every request's subject in the snapshot's hot hashed class (DevGraph::hot_*; {0, 1}, the reserved empty bucket, where the
    // subject has no row there): what the deep levels gathered per ENTRY -- some 50 times per request -- is gathered once per request, at the seeds
    __shared__ uint2 s_sd[E8 ? WAVES * 64 : 1];
    __shared__ uint8_t s_has[E8 ? WAVES * 64 : 1], s_err[E8 ? WAVES * 64 : 1];  // E8: the unit's answer bytes (ans_get / ans_set)
    if (E8) {
        has = s_has;
        err = s_err;
    }
    extern __shared__ uint4 s_prog[];  // dynamic: sized by the launcher to THIS snapshot's program table (a fixed 8 KiB cost two blocks per CU)
    const SlotProg *progs;
    const FwdOp *ops;
    load_programs<LDSPROG>(g, s_prog, progs, ops, WAVES * 64);
    CombineOut co;  // the block's own region of nodes and leaf cells
    if (CMB) co = CombineOut{g.nodes + (size_t)blockIdx.x * g.node_cap, &s_ccount[1], &s_ccount[0], g.node_cap, g.cell_cap, g.cell0 + blockIdx.x * g.cell_cap, 1u, g.bexpr};
    const uint32_t lane = lane_id();
    const uint32_t wib = uniform(threadIdx.x >> 6);  // (wave-uniform, and the compiler is told so: per-wave pointers then live in SGPRs)
    TaskLds &t = lds[wib];
    if (lane < kHeadWords) t.heads[lane] = 0ull;  // (flush_simple's head bits: zero between expansions)
    const DevShard nosh{};
    uint4 *bufs[2] = {buf0 + (size_t)blockIdx.x * cap, buf1 + (size_t)blockIdx.x * cap};
    if (lane == 0) {
        s_cold[wib] = WaveOutCold{};
        s_cold[wib].overflow = overflow;
        s_cold[wib].cap = E8 ? 2u * cap : cap;  // (the block's region holds twice as many 8-byte entries)
#if ACL_PROFILE_PHASES
        s_cold[wib].last = (uint32_t)__builtin_amdgcn_s_memtime();
#endif
    }
    if (threadIdx.x == 0) s_stop = 0;
    WaveOut wo;
    wo.cur = 0;
    wo.fill = 0;
    wo.produced = 0;
    wo.cold = &s_cold[wib];
    wo.lcap = E8 ? 2u * cap : cap;  // (the block's region holds twice as many 8-byte entries)
    wo.lfill = &s_fill[1];
    wo.ssd = s_sd;
    // units [0, nstatic) hold rpw requests each (block b starts on unit b: no hand-out); the requests behind them come in SMALL units of rdyn,
    // handed out through `next_unit` as blocks finish -- the launch's tail is then a small unit's walk, not the slowest big unit's
    const uint32_t nstat_req = min(n, nstatic * rpw);
    for (uint32_t unit = blockIdx.x; unit < nunits;) {
        // skew != 0 (host-mapped batches of a lone caller, static units only): the items cross PCIe in block order, so block u's seeds arrive
        // ~ u / nunits of the transfer late -- unit u gets rpw + skew (first block) ... rpw - skew (last) requests, and the blocks end together
        // instead of the last ones trailing by the transfer time: boundary(u) = u rpw + skew u (nunits - u) / nunits, `skew` in 1/256ths per unit
        uint32_t first = unit < nstatic ? unit * rpw : nstat_req + (unit - nstatic) * rdyn;
        uint32_t mine = unit < nstatic ? min(rpw, nstat_req - first) : min(rdyn, n - first);  // <= WAVES * 64: thread i seeds and answers request first + i
        if (skew) {
            const uint32_t u = uniform(unit);
            first = min(n, u * rpw + ((skew * u * (nunits - u)) >> 8));
            mine = min(n, (u + 1u) * rpw + ((skew * (u + 1u) * (nunits - u - 1u)) >> 8)) - first;
        }
        if (threadIdx.x < kCursorWords) s_cursors[threadIdx.x] = 0;
        if (CMB && threadIdx.x < 2) s_ccount[threadIdx.x] = 0;
        __syncthreads();
        // ---- seeds (k_seed's validation), in registers: wave w holds requests [64 w, 64 w + 64) of the unit
        const bool valid = threadIdx.x < mine;
        const uint32_t req = first + threadIdx.x;
        uint4 e = make_uint4(0, 0, kDeadMeta, 0);
        if (valid) {
            // (items == nullptr: a batch of <= 4 items rides in the kernel's arguments -- a single check's item does not cost a trip across PCIe)
            uint4 it;
            if (items) {  // (uniform)
                it = gld(items, req);
            } else {
                const uint32_t qi = req & 3u;
                it = qi == 0u ? inl.v[0] : (qi == 1u ? inl.v[1] : (qi == 2u ? inl.v[2] : inl.v[3]));
            }
            const uint32_t rtype = it.x & 0xFFFFu, perm = it.x >> 16, stype = it.z & 0xFFFFu, srel = it.z >> 16;
            const bool tok = rtype < g.ntypes && stype < g.ntypes;
            const uint32_t rt = tok ? rtype : 0u, st = tok ? stype : 0u;
            const uint32_t rmem = gld(g.type_nmembers, rt), smem = gld(g.type_nmembers, st), rbase = gld(g.type_slot_base, rt), sbase = gld(g.type_slot_base, st);
            const bool ok = tok && perm < rmem && (srel == 0xFFFFu || srel < smem);
            ans_set<E8>(has, req, first, 0);
            ans_set<E8>(err, req, first, (uint8_t)(ok ? ITEM_ERR_NONE : ITEM_ERR_INVALID));
            const uint32_t skey = srel == 0xFFFFu ? g.nslots + stype : sbase + srel;
            const uint32_t meta = ok ? make_meta(rbase + perm, 1u, skey) : kDeadMeta;
            e = make_uint4(it.y, req, meta, it.w);
            if (E8) {
                s_req[threadIdx.x] = make_uint2(it.w, skey);
                uint2 sd = make_uint2(0u, 1u);
                if (g.hot_cnrows) {  // (uniform)
                    const bool hot = skey == g.hot_ckey && it.w < g.hot_cnrows;
                    const uint2 d = gld(reinterpret_cast<const uint2 *>(g.meta), g.hot_cbase + (hot ? it.w : 0u));
                    if (hot && d.y != 0u) sd = d;
                }
                s_sd[threadIdx.x] = sd;
            }
        }
        wo.first = first;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        uint32_t level_reached = 1;
        wo.buf = bufs[0];
        wo.cur = 0;
        wo.lfill = &s_fill[1];  // level 1
        ACL_MARK(wo, PH_SEED);
        {
            NoNext nn;
            co.iter = 1u;
            process_segment<false, true, CMB, NoNext, true>(e, valid, nn, t, wo, lane, g, progs, ops, has, err, nosh, co);
        }
        uint32_t parity = 0;
        for (uint32_t level = 2; level <= kMaxLevels + 1; level++) {
            // ---- level boundary: everybody's children are written, the cursors turn over
            if (wo.cur == kNoSpace && lane == 0) s_stop = 1;  // overflow: the host redoes the batch
            __syncthreads();
            const uint32_t cnt = s_fill[(level - 1) % 3];
            const bool stop = s_stop != 0;
            if (threadIdx.x == 0) {
                s_fill[(level + 1) % 3] = 0;
                s_next[(level + 1) % 3] = 0;
            }
            ACL_MARK(wo, PH_BARRIER);
            if (stop || !cnt) break;
            level_reached = level;
            wo.lfill = &s_fill[level % 3];
            uint32_t *const next_seg = &s_next[level % 3];
            LocalWalk<E8> lw{bufs[parity], cnt, 0u, lane, false, s_req, first};
            parity ^= 1u;
            wo.buf = bufs[parity];
            co.iter = level;
            // Segments are claimed in PAIRS: one prologue and one set of trips for 128 entries.  (Claiming a level's last segments one by one was tried
            // and was slower: profiles/r05_ab_seeded_rows.txt.)
            const uint32_t nseg = (cnt + 63u) >> 6;
            if (E8) {
                // ---- the NEXT pair's entries travel while the current pair is expanded (round 6).  A pair's walk is a chain of dependent trips -- its entries,
                // the parents' descriptors, then edges and buckets per step -- and the first of them, the entries (an L2 hit: this block wrote them a level
                // ago), was a tenth of the walk's wave-time (profiles/r04_phases_final.txt "entries wait").  A wave now claims pair k + 1 and issues the
                // loads of its 128 raw 8-byte entries (4 VGPRs) BEFORE it expands pair k; they are decoded when their turn comes.  Claiming ahead
                // is only done while at least a round of pairs is still unclaimed: a pair held by a busy wave while other waves stand at the level
                // barrier would lengthen the level's tail (the last WAVES pairs are claimed the old way, when their wave is free).
                auto claim = [&]() -> uint32_t {
                    uint32_t c = 0;
                    if (lane == 0) c = atomicAdd(next_seg, 1u);
                    return 2u * uniform(c);
                };
                auto fetch = [&](uint32_t sgp, uint2 &ra, uint2 &rb) {
                    const uint32_t last = cnt - 1u;
                    ra = lw.raw(min(sgp * 64u + lane, last));
                    rb = lw.raw(min(sgp * 64u + 64u + lane, last));
                };
                uint32_t sg = claim();
                uint2 rA = make_uint2(0u, 0u), rB = rA;
                if (sg < nseg) fetch(sg, rA, rB);
                while (sg < nseg) {
                    uint32_t sgn = nseg;
                    uint2 nA = make_uint2(0u, 0u), nB = nA;
                    const uint32_t seen = uniform(__hip_atomic_load(next_seg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
                    const bool ahead = 2u * (seen + (uint32_t)WAVES) < nseg;
                    if (ahead) {
                        sgn = claim();
                        if (sgn < nseg) fetch(sgn, nA, nB);
                    }
                    {
                        lw.s = sg;
                        lw.second = true;
                        lw.rawB = rB;
                        lw.have_rawB = true;
                        const bool v = sg * 64u + lane < cnt;
                        process_segment<false, true, CMB>(decode_entry8(rA, s_req, first), v, lw, t, wo, lane, g, progs, ops, has, err, nosh, co);
                        if (lw.second && (sg + 1u) * 64u < cnt) {  // the pair's second segment did not go with the first
                            lw.s = sg + 1u;
                            lw.second = false;
                            const bool vb = (sg + 1u) * 64u + lane < cnt;
                            process_segment<false, true, CMB>(decode_entry8(rB, s_req, first), vb, lw, t, wo, lane, g, progs, ops, has, err, nosh, co);
                        }
                    }
                    if (!ahead) {
                        sgn = claim();
                        if (sgn < nseg) fetch(sgn, nA, nB);
                    }
                    sg = sgn;
                    rA = nA;
                    rB = nB;
                }
            } else {  // (the combine instantiations' 16-byte entries: a pair is claimed and its entries loaded when the wave is free)
                for (;;) {
                    uint32_t sg = 0;
                    if (lane == 0) sg = atomicAdd(next_seg, 1u);
                    sg = uniform(sg);
                    const uint32_t take = sg < nseg ? 2u : 1u;
                    sg = sg < nseg ? 2u * sg : nseg + sg;  // (claim c is the pair of segments 2 c, 2 c + 1; a claim beyond the level's pairs ends the loop)
                    if (sg >= nseg) break;
                    for (lw.s = sg, lw.second = take > 1u; lw.s < sg + take && lw.s * 64 < cnt; lw.s++) {
                        if (lw.s > sg && !lw.second) break;  // the pair's second segment went with the first
                        const bool v = lw.s * 64 + lane < cnt;
                        const uint4 en = lw.at(v ? lw.s * 64 + lane : lw.s * 64);  // unconditional; process_segment masks by `v`
                        if (lw.s > sg) lw.second = false;
                        process_segment<false, true, CMB>(en, v, lw, t, wo, lane, g, progs, ops, has, err, nosh, co);
                    }
                }
            }
        }
        // (statistics: dispatch levels the deepest request of the batch needed.  Test before the atomic: 2 048 blocks ending together on
        //  one address serialise at ~12 ns each -- C2's 18 us kernel took 38 us with an unconditional atomicMax.)
        if (max_level && threadIdx.x == 0 && level_reached > __hip_atomic_load(max_level, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(max_level, level_reached);
        // ---- combine nodes: deepest iteration first (a node's leaves are answered by the walk and by nodes of LATER iterations only)
        if (CMB) {
            __syncthreads();
            const uint32_t nn = min(s_ccount[1], co.node_cap);
            if (nn && !s_stop) {
                for (uint32_t it = level_reached; it >= 1u; it--) {
                    for (uint32_t ph = 0; ph < 2u; ph++) {  // the member nodes of intersection arrows first: the regular nodes of `it` read what they fold
                        for (uint32_t i = threadIdx.x; i < nn; i += WAVES * 64) {
                            const uint4 nd = co.nodes[i];
                            if ((nd.z >> 16) != it || (nd.w != 0u) != (ph == 0u)) continue;
                            if (ph == 0u) resolve_member(nd, has, err);
                            else resolve_node(nd, progs, co.bexpr, has, err);
                        }
                        __syncthreads();
                    }
                }
            }
        }
        // ---- answers (k_finalize): every wave's has[] / err[] stores are behind a block barrier
        __syncthreads();
        if (valid) {
            const bool h = E8 ? s_has[threadIdx.x] != 0 : __hip_atomic_load(has + req, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != 0;
            const uint8_t er = h ? (uint8_t)ITEM_ERR_NONE : (E8 ? s_err[threadIdx.x] : __hip_atomic_load(err + req, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
            perm_out[req] = h ? 2 : (er ? 0 : 1);
            if (err_out) err_out[req] = er == ITEM_ERR_DEPTH ? 100 : (er == ITEM_ERR_INVALID ? 9 : 0);
        }
        if (s_stop || !next_unit) break;
        if (threadIdx.x == 0) s_unit = gridDim.x + atomicAdd(next_unit, 1u);
        __syncthreads();
        unit = s_unit;
    }
#if ACL_PROFILE_PHASES
    ACL_MARK(wo, PH_OTHER);
    if (lane < 20) atomicAdd(&acl_phase_cycles[lane], (unsigned long long)s_cold[wib].prof[lane]);
#endif
    // ---- small host batches (round 5): the caller does not wait in hipStreamSynchronize -- that costs ~5.5 us AFTER the kernel's
    // last store is visible to a spinning host thread (tools/launch_latency.hip: flag visible 6.6 us after the launch call, synchronize returns at
    // 11.9-15 us) -- it spins on `done_flag`, a word of pinned host memory that the LAST block to finish sets.  Every block releases its answers
    // (stores into host memory) at system scope before it arrives at the device counter; the last arrival re-arms the counter and raises the flag.
    if (done_flag) {
        __syncthreads();  // (every wave's answer stores are issued)
        if (threadIdx.x == 0) {
            __threadfence_system();
            if (__hip_atomic_fetch_add(done_ctr, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u) {
                __hip_atomic_store(done_ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(done_flag, done_val, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

// Merges identical pending sub-checks of one level: two frontier entries with the same (request, state, level) have identical
// subtrees, so all but one are struck (meta = dead) -- answers cannot change.  Only run when a pass outgrew its frontier: on
// sane graphs duplicates are rare (1.8 % on C4, profiles/r02_c4_duplicate_ratio.txt) and the walk is faster without it, but group
// nesting with BRANCHING cycles (g0 -> {g0, g1}, g1 -> g0) doubles the frontier every level for 50 levels; SpiceDB's
// dispatcher cuts the same recursion at depth 50, and the oracle memoises on exactly this key.
// key = request[14] | level[6] | slot[13] | object id[31] (dedup passes run on slices of <= 16 384 requests); table: open
// addressing over u64, empty = ~0.
__global__ __launch_bounds__(256) void k_dedup(DevFrontier f, uint32_t iter, unsigned long long *table, uint32_t bits) {
    uint4 *buf = f.buf[iter & 1u];
    const uint32_t *counts = f.counts[iter & 1u];
    if (*f.overflow) return;
    const uint32_t C = f.nwaves + min(f.nchunks[iter], f.max_chunks - f.nwaves);
    const uint32_t mask = (1u << bits) - 1u;
    for (uint32_t c = blockIdx.x; c < C; c += gridDim.x) {
        const uint32_t cnt = counts[c];
        for (uint32_t i = threadIdx.x; i < cnt; i += blockDim.x) {
            const uint4 e = buf[(size_t)c * kChunk + i];
            if (e.z == kDeadMeta) continue;
            const unsigned long long key = ((unsigned long long)(e.y & 0x3FFFu) << 50) | ((unsigned long long)meta_level(e.z) << 44) |
                                           ((unsigned long long)meta_slot(e.z) << 31) | (unsigned long long)(e.x & kIdMask);
            uint32_t h = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> (64 - bits));
            for (;;) {
                const unsigned long long old = atomicCAS(table + h, ~0ull, key);
                if (old == ~0ull) break;  // first of its kind
                if (old == key) {
                    buf[(size_t)c * kChunk + i].z = kDeadMeta;
                    break;
                }
                h = (h + 1u) & mask;
            }
        }
    }
}

// The same for schemas with `&` / `-`, whose entries carry a result CELL (32 bits) where the request was: cell | object id is the 64-bit key
// of the table, level | slot sits in a second table the slot's winner fills right behind its CAS -- a lane that meets its own first half
// reads the second one, and comes back in the next round while it is still empty (the winner has left the loop by then: no lane ever waits
// for a lane of its own wave).  Identical (cell, state, level) entries have identical subtrees AND identical combine nodes to create, so
// all but one are struck before any node exists.
__global__ __launch_bounds__(256) void k_dedup_cells(DevFrontier f, uint32_t iter, unsigned long long *table, uint32_t *second, uint32_t bits) {
    uint4 *buf = f.buf[iter & 1u];
    const uint32_t *counts = f.counts[iter & 1u];
    if (*f.overflow) return;
    const uint32_t C = f.nwaves + min(f.nchunks[iter], f.max_chunks - f.nwaves);
    const uint32_t mask = (1u << bits) - 1u;
    for (uint32_t c = blockIdx.x; c < C; c += gridDim.x) {
        const uint32_t cnt = counts[c];
        for (uint32_t i = threadIdx.x; i < cnt; i += blockDim.x) {
            const uint4 e = buf[(size_t)c * kChunk + i];
            if (e.z == kDeadMeta) continue;
            const unsigned long long key = ((unsigned long long)e.y << 32) | (unsigned long long)(e.x & kIdMask);  // (bit 31 clear: never the empty mark)
            const uint32_t rest = 1u + (e.z & 0x7FFFFu);                                                           // level | slot, never 0
            uint32_t h = (uint32_t)(((key ^ ((unsigned long long)rest << 40)) * 0x9E3779B97F4A7C15ull) >> (64 - bits));
            for (;;) {
                const unsigned long long old = atomicCAS(table + h, ~0ull, key);
                if (old == ~0ull) {  // first of its kind: publish the second half
                    __hip_atomic_store(second + h, rest, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                    break;
                }
                if (old == key) {
                    const uint32_t r2 = __hip_atomic_load(second + h, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
                    if (r2 == 0u) continue;  // the winner is between its CAS and its store: look again
                    if (r2 == rest) {
                        buf[(size_t)c * kChunk + i].z = kDeadMeta;
                        break;
                    }
                }
                h = (h + 1u) & mask;
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_finalize(uint32_t n, const uint8_t *__restrict__ has, const uint8_t *__restrict__ err, uint8_t *perm_out,
                                                   int32_t *err_out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool h = has[i];
    const uint8_t e = h ? (uint8_t)ITEM_ERR_NONE : err[i];
    perm_out[i] = h ? 2 : (e ? 0 : 1);
    if (err_out) err_out[i] = e == ITEM_ERR_DEPTH ? 100 : (e == ITEM_ERR_INVALID ? 9 : 0);
}

// Level loop, schemas with `&` / `-`: the combine nodes of ONE frontier iteration (launched for iter = last .. 1; the list is scanned whole
// every time -- this is the overflow path, not the fast one).
__global__ __launch_bounds__(256) void k_resolve(DevGraph g, uint32_t iter, uint32_t members, uint8_t *has, uint8_t *err) {
    const uint32_t nn = min(g.ccount[1], g.node_cap);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nn; i += gridDim.x * blockDim.x) {
        const uint4 nd = g.nodes[i];
        if ((nd.z >> 16) != iter || (nd.w != 0u) != (members != 0u)) continue;
        if (members) resolve_member(nd, has, err);  // (launched first: the regular nodes of the iteration read what the members fold)
        else resolve_node(nd, g.progs, g.bexpr, has, err);
    }
}

// Sharded graph, schemas with `&` / `-` (round 5): every shard appended the combine nodes of the states IT visited; after the walk the node lists are
// all-gathered (world blocks of `stride` nodes, block b holding hdrs[b].x of them) and, has / err being identical on every shard by then (a
// byte-wise max over the whole cell space), every shard resolves ALL nodes -- redundantly and identically, so no cell has to travel between
// the resolve iterations.
__global__ __launch_bounds__(256) void k_resolve_gathered(DevGraph g, const uint4 *__restrict__ nodes, uint32_t stride, const uint4 *__restrict__ hdrs, uint32_t iter, uint32_t members,
                                                          uint8_t *has, uint8_t *err) {
    const uint32_t nn = min(hdrs[blockIdx.y].x, stride);
    const uint4 *__restrict__ mine = nodes + (size_t)blockIdx.y * stride;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nn; i += gridDim.x * blockDim.x) {
        const uint4 nd = mine[i];
        if ((nd.z >> 16) != iter || (nd.w != 0u) != (members != 0u)) continue;
        if (members) resolve_member(nd, has, err);
        else resolve_node(nd, g.progs, g.bexpr, has, err);
    }
}
__global__ void k_node_hdr(uint4 *hdr, const uint32_t *ccount) { *hdr = make_uint4(ccount[1], ccount[0], 0u, 0u); }  // {nodes appended, cells handed out}

// Post-filter hand-off (reference pkg/authz/postfilter.go:144-178): list item i owns the bulk-check pairs
// [item_off[i], item_off[i+1]); it is kept iff every one of them is HAS_PERMISSION without error -- an item
// with no pairs (templates that did not resolve, postfilter.go:92-95,145-150) is kept.
__global__ __launch_bounds__(256) void k_keep(uint32_t k_items, const uint32_t *__restrict__ item_off, const uint8_t *__restrict__ perm, uint8_t *keep_out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= k_items) return;
    bool all = true;
    for (uint32_t j = item_off[i], e = item_off[i + 1]; j < e; j++) all = all && perm[j] == 2;  // PERMISSIONSHIP_HAS_PERMISSION
    keep_out[i] = all ? 1 : 0;
}

// ----------------------------------------------------------- reverse expand
// entry: x = object id, y = lookup request, z = meta (slot | dist << 13 | flags), w unused.
// dist == 0 marks a seed entry: slot field holds the SUBJECT KEY and the program is rseeds[key].
// PHASE: REV_FUSED  (unsharded) visit + expand in one pass;
//        REV_VISIT  (sharded)   test-and-set `visited`, pass first visits on (kRevVisited) and export the ones whose
//                               parent rows also live on other shards (kRevForeign) -- no expansion;
//        REV_EXPAND (sharded)   expand seeds / visited / foreign entries, never touching `visited`.
// Two phases keep the sharded walk level-synchronous: a state and its foreign copies are expanded in the same
// iteration, so "first visit wins" still records the minimum distance (the depth-50 cut depends on it).
template <uint32_t PHASE>
__global__ __launch_bounds__(kBlock, ACL_MIN_WAVES_PER_SIMD) void k_rev_expand(DevReverse r, DevFrontier f, uint32_t iter, DevShard sh) {
    __shared__ TaskLds lds[kWavesPerBlock];
    __shared__ WaveOutCold s_cold[kWavesPerBlock];
    const uint32_t lane = lane_id();
    const uint32_t wib = uniform(threadIdx.x >> 6);  // (wave-uniform, and the compiler is told so: per-wave pointers then live in SGPRs)
    TaskLds &t = lds[wib];
    const uint32_t wave = blockIdx.x * kWavesPerBlock + wib, nwaves = f.nwaves;
    const uint32_t pin = (iter + 1) & 1u;
    const uint4 *__restrict__ in = f.buf[pin];
    const uint32_t *__restrict__ in_counts = f.counts[pin];
    const bool live = !*f.overflow && f.any[iter - 1];
    const uint32_t C = live ? nwaves + min(f.nchunks[iter - 1], f.max_chunks - nwaves) : 0u;
    const DevGraph nog{};
    WaveOut wo = chunked_out(f, iter, wave, &s_cold[wib], lane);
    uint4 *__restrict__ out = wo.buf;
    // segment-major work order, as in k_expand (ChunkWalk)
    const uint32_t nslot = C * kSegsPerChunk;
    for (uint32_t x0 = wave; x0 < nslot; x0 += 64 * nwaves) {
        const uint32_t xl = x0 + lane * nwaves;
        uint32_t lc = 0, lcnt = 0;
        if (xl < nslot) {
            const uint32_t ls = xl / C;
            lc = (xl % C + ls * 509u) % C;
            lcnt = in_counts[lc];
            lcnt = lcnt > ls * 64 ? lcnt - ls * 64 : 0u;  // entries of this slot's segment and beyond
        }
        uint64_t work = __ballot(lcnt != 0);
        while (work) {
        const int wl = __ffsll((unsigned long long)work) - 1;
        work &= work - 1;
        const uint32_t x = x0 + (uint32_t)wl * nwaves;
        const uint32_t s = x / C, c = (uint32_t)__builtin_amdgcn_readlane((int)lc, wl);
        const uint32_t cnt = (uint32_t)__builtin_amdgcn_readlane((int)lcnt, wl) + s * 64;
        const bool valid = s * 64 + lane < cnt;
        const uint4 e = valid ? gld(in, c * kChunk + s * 64 + lane) : make_uint4(0, 0, kDeadMeta, 0);
        const uint32_t id = e.x, req = e.y, meta = e.z;
        bool active = valid && meta != kDeadMeta;
        const uint32_t slot = meta & 0x1FFFu, dist = (meta >> 13) & 63u;
        RevProg p{0, 0};
        bool first_visit = false;
        if (active) {
            if (dist == 0) {
                p = r.rseeds[slot];
            } else if (PHASE == REV_EXPAND) {
                p = r.rprogs[slot];  // kRevVisited or kRevForeign: the visit already happened (here or on the owner)
            } else if (id < r.slot_nobjects[slot]) {
                // first visit wins: level-synchronous order makes it the minimum distance
                const uint32_t bit = r.slot_bit_base[slot] + id;
                const uint32_t m = 1u << (bit & 31u);
                const uint32_t old = atomicOr(r.visited + (size_t)req * r.visited_words + (bit >> 5), m);
                if (old & m) active = false;
                else {
                    p = r.rprogs[slot];
                    first_visit = true;
                }
            } else {
                active = false;
            }
        }
        if (PHASE == REV_VISIT) {
            // seeds and first visits move on to the expand phase; states with parents elsewhere are also exported
            const uint4 o = make_uint4(id, req, first_visit ? (meta | kRevVisited) : meta, 0);
            const uint64_t b = __ballot(active);
            if (b) {
                const uint32_t base = reserve<false>(wo, (uint32_t)__popcll(b), lane);
                if (active && base != kNoSpace) out[base + lanes_below(b)] = o;
            }
            const bool xport = first_visit && (p.n & kRevRemoteBit) && dist < kMaxLevels;
            const uint4 xe = make_uint4(id, req, meta | kRevForeign, 0);
            if (!sh.by_dest) {
                export_entries(xport, xe, 0u, lane, sh);  // one block every shard receives; the importers keep what they hold parent rows for
            } else {
                // all-to-all form: a copy into the block of every shard that holds parent rows of this slot's states -- one round per distinct
                // destination among the lanes' lowest pending bits (a slot has one or two such shards; rounds = the wave's distinct destinations)
                uint64_t pend = xport ? r.rdest[slot] : 0ull;
                while (__ballot(pend != 0)) {
                    const uint32_t d = pend ? (uint32_t)(__ffsll((unsigned long long)pend) - 1) : 0u;
                    export_entries(pend != 0, xe, d, lane, sh);
                    pend &= pend - 1;
                }
            }
            continue;
        }
        const uint32_t nops = (active && dist < kMaxLevels) ? (p.n & ~kRevRemoteBit) : 0u;  // parents of a dist-50 state would need 51 levels
        uint32_t T = 0;
        const uint32_t maxops = uniform(wave_max(nops));
        for (uint32_t j = 0; j < maxops; j++) {
            bool want = false;
            uint32_t tstart = 0, tcount = 0, tmeta = 0;
            if (j < nops) {
                const RevOp op = r.rops[p.first + j];
                const bool dead = op.target < 256u && !((r.useful[op.target >> 5] >> (op.target & 31u)) & 1u);  // (cannot lead to the result slot: DevReverse::useful)
                if (dead) {
                } else if (op.flags & OP_PUSH_SAME) {
                    want = true;
                    tstart = id;
                    tcount = 1u | kSelfBit;
                } else if ((op.flags & OP_WILD) || id < op.nrows) {  // (OP_WILD, seeds only: the wildcard subject's row, whatever the seed's id)
                    const uint2 rd = reinterpret_cast<const uint2 *>(r.rmeta)[op.roff_base + ((op.flags & OP_WILD) ? 0u : id)];
                    const uint32_t s0 = rd.x, s1 = rd.y;
                    if (s1 - s0 > kMaxRow) *f.overflow = 2u;
                    else if (s1 > s0) {
                        want = true;
                        tstart = s0;
                        tcount = s1 - s0;
                    }
                }
                tmeta = op.target | ((dist + 1) << 13);
            }
            const uint64_t b = __ballot(want);
            if (b) {
                if (want) {
                    const uint32_t q = T + lanes_below(b);
                    t.a[q] = make_uint4(tstart, 0u, 1u, req);
                    t.count[q] = tcount;
                    t.meta[q] = tmeta;
                    t.sid[q] = 0;
                }
                T += (uint32_t)__popcll(b);
                if (T > kTaskCap - 64) {
                    flush_tasks<false, false, false>(t, T, wo, lane, nog, nullptr, nullptr, r.redges, nullptr, nullptr, sh);
                    T = 0;
                }
            }
        }
        if (T) flush_tasks<false, false, false>(t, T, wo, lane, nog, nullptr, nullptr, r.redges, nullptr, nullptr, sh);
        }
    }
    if (lane == 0) {
        if (wo.cur != kNoSpace) wo.cold->counts[wo.cur] = wo.fill;
        if (wo.produced) f.any[iter] = 1u;
    }
}

// ------------------------------------------------------- reverse walk, single launch
// LookupResources as the proxy issues it: one request per list call (reference pkg/authz/lookups.go:49-83), a few dozen in flight
// (one goroutine per request: responsefilterer.go:165-204).  The level loop above costs one k_rev_expand launch per reverse level plus a
// status round trip, whatever the batch size, and writes every result id through the frontier once more before the next launch sets
// its bit (the level that produces the ~10 k result pods of a C3 lookup is the children of ~100 namespace entries).  Here ONE launch
// answers the batch: block b walks lookup b through every reverse level by itself.
//   * entries of a level = true states (object id, slot); their distance is the level: uniform, not stored;
//   * phase A: every thread takes an entry and turns its program's ops into tasks (row start, degree, target) in an LDS list
//     (computed-userset parents -- PUSH_SAME -- are visited right there);
//   * phase B: a block-wide prefix sum over the degrees, then the 1024 lanes walk the OUTPUT index space: lane -> task by a binary
//     search over the LDS prefix array, consecutive lanes read consecutive resource ids of a reverse row (coalesced), four children
//     per lane in flight;
//   * a child is VISITED WHERE IT IS PRODUCED: test-and-set of its bit in the request's visited bitmap (first visit wins; everything
//     produced in one level has the same distance, so "first" is still "nearest" -- the depth-50 cut depends on it).  Children whose
//     slot has no parents (the lookup's own result slot, typically) need no answer from the atomic and are never written anywhere
//     else: the bit IS the result.  Only first visits of states that do have parents enter the block's private frontier region.
//   * the block zeroes its own bitmap at the start and, at the end, copies the result slot's words to the caller's rows (device,
//     or pinned host memory: no separate D2H copy) and counts the ids.
// A block that outgrows its region or meets a level of more than kRevLocalBudget children raises `overflow`: the host redoes the
// batch on the level loop, which spreads one huge lookup over the whole chip.
constexpr int kRevLocalThreads = 1024;
constexpr uint32_t kRevTaskCap = kRevLocalThreads;  // one (state, op) pair per thread and round => at most one task per thread
constexpr uint32_t kRevLocalBudget = 1u << 22;      // children of one round a single block may enumerate
constexpr uint32_t kRevTerminal = 0x80000000u;      // task target flag: children are only marked, never expanded
constexpr uint32_t kRevNoMark = 0x40000000u;        // task target flag (OP_NOMARK seed ops): every child is a first visit by construction -- no visited bit
constexpr uint32_t kRevIsTarget = 0x20000000u;      // task target flag (k_rev_multi): the child's slot is one of the launch's targets -- always marked
constexpr uint32_t kRevTaskFlags = kRevTerminal | kRevNoMark | kRevIsTarget;
constexpr uint32_t kRevNoTask = 0xFFFFFFFFu;        // a policy's answer for an op that has nothing to enumerate at this level (no slot carries all three flags)
constexpr uint32_t kRevNoSlot = 0xFFFFFFFFu;

// ---- block primitives of the one-block walks (k_rev_local and k_rev_multi through rev_block_walk; k_subj_local, k_explain_local and k_reach_local through
// subj_block_walk)
// Block-wide exclusive scan of one degree per thread: before = the sum over the threads below this one, total = the block's sum (block-uniform).
// One barrier, between the store of the wave totals and their read; a caller that scans again puts a barrier of its own between the two.
template <int THREADS>
__device__ __forceinline__ void block_excl_scan(uint32_t deg, uint32_t lane, uint32_t wib, uint32_t *s_wave_tot, uint32_t &before, uint32_t &total) {
    const uint32_t incl = wave_incl_scan(deg, lane);
    if (lane == 63) s_wave_tot[wib] = incl;
    __syncthreads();
    before = incl - deg;
    total = 0;
#pragma unroll
    for (uint32_t w = 0; w < THREADS / 64; w++) {
        const uint32_t wt = s_wave_tot[w];
        before += w < wib ? wt : 0u;
        total += wt;
    }
}
// Wave-cooperative append of the flagged lanes' entries (uint2 or uint4) to the block's log of `cap` entries, whose end lives in LDS.  A wave that does not
// fit raises *s_stop = 1 and stores nothing.  Call in wave-uniform control flow.
template <typename E>
__device__ __forceinline__ void log_append(E *log, uint32_t cap, uint32_t *s_end, uint32_t *s_stop, uint32_t lane, bool push, const E &e) {
    const uint64_t b = __ballot(push);
    if (!b) return;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(s_end, (uint32_t)__popcll(b));
    base = uniform(base);
    if (base + (uint32_t)__popcll(b) > cap) {
        if (lane == 0) *s_stop = 1u;
        return;
    }
    if (push) log[base + lanes_below(b)] = e;
}
// The task that owns output index w: the last of CAP tasks whose exclusive prefix is <= w (threads without a task have degree 0, so it is never one of them)
template <uint32_t CAP>
__device__ __forceinline__ uint32_t task_owner(const uint32_t *prefix, uint32_t w) {
    uint32_t jt = 0;
#pragma unroll
    for (uint32_t step = CAP / 2; step >= 1; step >>= 1)
        if (prefix[jt + step] <= w) jt += step;
    return jt;
}

struct RevTaskLds {
    uint32_t start[kRevTaskCap];       // first resource id of the row in `redges`
    uint32_t prefix[kRevTaskCap + 1];  // exclusive prefix of the degrees (a thread without a task: degree 0)
    uint32_t target[kRevTaskCap];      // child slot | kRevTerminal
};
struct RevProgLds {  // the reverse programs, staged once per block (the host only takes this path when they fit)
    RevOp ops[kRevLdsOps];
    RevProg progs[kRevLdsSlots];
    uint2 slot[kRevLdsSlots];  // {first bit of the slot's visited rows, id space they cover}
};
struct RevWalkLds {  // the static LDS both reverse one-block kernels declare, alignas(16) (rev_stage_programs sets it up, rev_block_walk runs on it)
    uint32_t wave_tot[kRevLocalThreads / 64];  // block_excl_scan's, and block_count's behind the walk (first: read back as four 16-byte loads)
    RevProgLds pl;  // (its 16-byte ops stay 16-byte aligned; the 3 073 words of `t` with the 11 below are a multiple of 8 bytes: no padding)
    RevTaskLds t;
    uint32_t end;                              // entries in the block's log
    uint32_t stop;                             // 1: redo on the level loop, 2: a row beyond kMaxRow; last writer wins, read only through the round's closing barrier
    uint32_t maxops;                           // the most parent ops any slot has: W of every level but the seed's
    uint32_t nomark[kRevLdsSlots / 32];        // slots whose states carry no visited bit in this launch (nothing to clear afterwards)
};

// A small batch's caller spins on `done_flag` (pinned host memory) instead of synchronising the stream (see k_check_local): every block releases
// what it stored into host memory at system scope, arrives at the device counter, and the last arrival re-arms the counter and raises the flag.
__device__ __forceinline__ void signal_done(uint32_t *done_ctr, uint32_t *done_flag, uint32_t done_val) {
    if (!done_flag) return;
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence_system();
        if (__hip_atomic_fetch_add(done_ctr, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u) {
            __hip_atomic_store(done_ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(done_flag, done_val, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// Round 6 -- BIG result types (rows beyond the block's LDS: the 8.45 M pods of BASELINE configs[4]'s graph, a 1 MB row).  One block enumerated every child of
// such a lookup -- 100-200 k pods under a few hundred namespaces and groups -- at ~5.5 ns each: 0.65-1.2 ms per lookup (profiles/r06_lookup_big.txt), and the
// level loop, which spreads a lookup over the chip, pays ~80 us per level for it.  What makes these lookups heavy is almost entirely TERMINAL: children in the
// lookup's own result slot, which are marked and never expanded -- no first-visit answer is needed, no order, no frontier.  So with `dfr.tasks` given the block
// does not enumerate such rows when a round holds `min_children` children or more: it appends {first edge, degree} to the lookup's DEFERRED list and walks on;
//   k_rev_terminal  (the next launch on the stream, blocks all over the chip) marks the deferred rows' ids in the lookup's result row -- a kernel boundary
//                   later, so the block's workgroup-scope marks are in memory and agent-scope atomics from every XCD meet them there;
//   k_rev_rows      (the launch after) copies the rows out slice by slice from all CUs, counts the ids, clears the slices it copied -- the three things that
//                   cost one block 80 us per lookup -- and the last block to finish hands the counts over and raises the caller's completion word.
struct RevDefer {
    uint2 *tasks = nullptr;      // [lookups][cap] {first edge, degree}; nullptr: nothing is deferred and the block copies its row itself (rows in LDS)
    uint32_t *count = nullptr;   // [lookups] tasks appended (zeroed by the block)
    uint32_t *levels = nullptr;  // [lookups] reverse levels walked (statistics; k_rev_rows packs them into the counts)
    uint32_t cap = 0;
    uint32_t min_children = 4096;  // children of one round from which its terminal rows go to the chip-wide launch (below: the block is done with them sooner than a launch starts)
    // The marks themselves are BYTES, not bits: one byte per object of the result type, [lookups][bm_stride], zero between launches.  Marking 100-200 k ids with
    // atomic ORs -- workgroup scope from one CU (round 5) or agent scope from all of them (this round's first version) -- ran at ~5 ns per id either way
    // (profiles/r06_lookup_big.txt): the read-modify-write is the cost.  A result slot nobody expands needs no answer from the mark, so a plain byte store does
    // (idempotent, no neighbour to lose); k_rev_rows folds 32 bytes into a word of the caller's row and zeroes the bytes it found set.
    uint8_t *bytemap = nullptr;
    uint32_t bm_stride = 0;
};

// ---- the setup, the walk and the clean-up k_rev_local and k_rev_multi share: each kernel is setup, rev_block_walk with its policy, epilogue
// Zeroes the walk's words and stages the reverse programs once per block (the host only takes these kernels when they fit): ops whose target slot cannot lead
// to a result slot are dead for this launch (`useful`: Snapshot::rev_useful -- a lookup of pod#creator does not walk the user's groups).  The caller puts a
// barrier between this and the first read of what was staged.
__device__ __forceinline__ void rev_stage_programs(const DevReverse &r, const RevUseful &useful, RevWalkLds &w, uint32_t tid) {
    if (tid == 0) {
        w.end = 0;
        w.stop = 0;
        w.maxops = 0;
    }
    if (tid < kRevLdsSlots / 32) w.nomark[tid] = 0;
    __syncthreads();
    for (uint32_t i = tid; i < r.nrops; i += kRevLocalThreads) {
        RevOp o = r.rops[i];
        if (o.target < kRevLdsSlots && !((useful.w[o.target >> 5] >> (o.target & 31u)) & 1u)) o.flags |= OP_DEAD;
        w.pl.ops[i] = o;
    }
    for (uint32_t i = tid; i < r.nslots; i += kRevLocalThreads) {
        const RevProg p = r.rprogs[i];
        w.pl.progs[i] = p;
        w.pl.slot[i] = make_uint2(r.slot_bit_base[i], r.slot_nobjects[i]);
        atomicMax(&w.maxops, p.n & ~kRevRemoteBit);
    }
}
// The slots whose states carry no visited bit: the targets of the seed's OP_NOMARK ops, but for result slots, whose states are always marked
template <typename F>
__device__ __forceinline__ void rev_build_nomark(const DevReverse &r, RevProg seed, RevWalkLds &w, uint32_t tid, F is_result_slot) {
    for (uint32_t i = tid; i < (seed.n & ~kRevRemoteBit); i += kRevLocalThreads) {
        const RevOp so = r.rops[seed.first + i];
        if ((so.flags & OP_NOMARK) && !is_result_slot(so.target)) atomicOr(&w.nomark[so.target >> 5], 1u << (so.target & 31u));
    }
}
// Leaves `visited` as it was handed over outside the result rows: every bit the block set there belongs to a logged first visit (whole words: they hold this
// lookup's bits only).  skip_slot: a slot whose marks live elsewhere or are cleared by someone else (kRevNoSlot: none).  Call behind a barrier.
__device__ __forceinline__ void rev_clear_logged(const RevWalkLds &w, const uint2 *log, uint32_t cap, uint32_t *__restrict__ visited, uint32_t tid, uint32_t skip_slot) {
    const uint32_t nlog = min(w.end, cap);
    for (uint32_t i = tid; i < nlog; i += kRevLocalThreads) {
        const uint2 en = log[i];
        if (en.y == skip_slot) continue;
        if (w.nomark[en.y >> 5] >> (en.y & 31u) & 1u) continue;  // (never marked)
        visited[(w.pl.slot[en.y].x + en.x) >> 5] = 0u;
    }
}
// Block-wide sum of one count per thread (a row holds < 2^31 ids), valid in thread 0.  One barrier, between the store of the wave totals and their read; a
// caller that counts again puts a barrier of its own between the two.
__device__ __forceinline__ uint32_t block_count(uint32_t c, uint32_t tid, uint32_t lane, uint32_t wib, uint32_t *s_wave_tot) {
    c = wave_last(wave_incl_scan(c, lane));
    if (lane == 0) s_wave_tot[wib] = c;
    __syncthreads();
    uint32_t tot = 0;
    if (tid == 0)
        for (uint32_t k = 0; k < kRevLocalThreads / 64; k++) tot += s_wave_tot[k];
    return tot;
}

// The level loop of one block: the frontier is ONE append-only log of first visits {id, slot} -- level L reads [lvl_lo, lvl_hi) and appends behind the end, so
// the log is also the list of what to clear afterwards (rev_clear_logged).  The seed (`sid` under the programs `seed`) is not in the log.  Per level, rounds of
// kRevLocalThreads (state, op) pairs: phase A turns a pair into at most one task and visits a same-object parent on the spot; a block-wide scan of the degrees;
// phase B walks the concatenated rows; each round closes with one __syncthreads_or of the stop word, the only way it is read.  Returns the block-uniform stop
// (0: the log ran dry or the depth limit was reached) and the reverse levels walked (by value: a reference would pin them in scratch memory).
// The policy P supplies what the two kernels do not share (its hooks run in wave-uniform control flow and contain no barrier):
//   target(op, level, term_all, pl)  the task target for an op at a level: slot | kRevTerminal | kRevNoMark | kRevIsTarget -- the kernel's own terminal rule and
//                                    mark-through -- or kRevNoTask when there is nothing to enumerate
//   visit(id, tgt, valid, pl)        marks child (slot, id); true when it was a first visit of a state that is expanded
//   kDefer, defers(tgt), dfr, ...    k_rev_local's deferral of a heavy round's terminal rows (see RevDefer); it holds a barrier, so it lives here, not in a hook
struct RevWalkEnd {
    int stop;
    uint32_t levels;
};
template <typename P>
__device__ __forceinline__ RevWalkEnd rev_block_walk(P &pol, const DevReverse &r, RevWalkLds &w, RevProg seed, uint32_t sid, uint2 *log, uint32_t cap, uint32_t tid,
                                                     uint32_t lane, uint32_t wib) {
    const uint2 *__restrict__ rmeta2 = reinterpret_cast<const uint2 *>(r.rmeta);
    const uint32_t *__restrict__ redges = r.redges;
    RevTaskLds &t = w.t;
    const RevProgLds &pl = w.pl;
    // wave-cooperative append to the block's log (call in wave-uniform control flow)
    auto append = [&](bool push, uint32_t id, uint32_t slot) { log_append(log, cap, &w.end, &w.stop, lane, push, make_uint2(id, slot)); };
    uint32_t lvl_lo = 0, cnt = 1;
    uint32_t level = 1;
    int stop = 0;  // block-uniform copy of w.stop (taken through a barrier: the word itself may be raised by a faster wave at any time)
    for (; level <= kMaxLevels; level++) {  // level L: states at distance L - 1 (all of them: uniform) produce children at distance L
        const uint2 *__restrict__ fin = log + lvl_lo;
        const uint32_t lvl_hi = lvl_lo + (level > 1 ? cnt : 0u);  // (the seed is not in the log)
        // a child at distance 50 is marked but never expanded (its parents would sit at 51): terminal whatever its slot
        const uint32_t term_all = level >= kMaxLevels ? kRevTerminal : 0u;
        // work items of a level = (state, op) pairs, one per thread and round: a seed's six rows, or the one or two parent ops of a
        // few hundred states, are fetched side by side instead of one after the other by the state's thread
        const uint32_t W = level == 1 ? (seed.n & ~kRevRemoteBit) : w.maxops;
        const uint32_t npairs = cnt * W;
        for (uint32_t pb = 0; pb < npairs; pb += kRevLocalThreads) {
            // ---- phase A: this thread's op -> at most one task (start, degree, target), kept in registers
            const uint32_t q = pb + tid;
            uint32_t deg = 0, start = 0, tgt = 0;
            bool same = false;  // computed-userset parent: the child is the same object
            uint32_t id = 0;
            if (q < npairs) {
                const uint32_t e = q / W, j = q - e * W;
                RevProg p = seed;
                id = sid;
                if (level > 1) {
                    const uint2 en = fin[e];
                    id = en.x;
                    p = pl.progs[en.y];
                }
                if (j < (p.n & ~kRevRemoteBit) && !(pl.ops[p.first + j].flags & OP_DEAD)) {
                    const RevOp op = pl.ops[p.first + j];
                    tgt = pol.target(op, level, term_all, pl);
                    if (tgt == kRevNoTask) {
                        tgt = 0u;  // nothing to enumerate for this op
                    } else if (op.flags & OP_PUSH_SAME) {
                        same = true;
                    } else if ((op.flags & OP_WILD) || id < op.nrows) {  // (OP_WILD, seeds only: the wildcard subject's row, whatever the seed's id)
                        const uint2 rd = rmeta2[op.roff_base + ((op.flags & OP_WILD) ? 0u : id)];
                        if (rd.y - rd.x > kMaxRow) w.stop = 2u;
                        else if (rd.y > rd.x) {
                            start = rd.x;
                            deg = rd.y - rd.x;
                        }
                    }
                }
            }
            {  // same-object parents are visited right here (wave-uniform control flow: the append ballots)
                const bool push = pol.visit(id, tgt, same, pl);
                append(push, id, tgt & ~kRevTaskFlags);
            }
            // ---- block-wide exclusive prefix of the degrees
            uint32_t before, total;
            block_excl_scan<kRevLocalThreads>(deg, lane, wib, w.wave_tot, before, total);
            if constexpr (P::kDefer) {
                const RevDefer &dfr = pol.dfr;
                if (dfr.tasks && total >= dfr.min_children) {  // (block-uniform) a heavy round: its terminal rows of the result slot go to the chip-wide launch
                    const bool mine = deg != 0u && pol.defers(tgt);
                    const uint64_t b = __ballot(mine);
                    if (b) {
                        uint32_t base = 0;
                        if (lane == 0) base = atomicAdd(pol.s_dfr, (uint32_t)__popcll(b));
                        base = uniform(base);
                        if (base + (uint32_t)__popcll(b) > dfr.cap) {
                            if (lane == 0) w.stop = 1u;  // (more rows than the list holds: the level loop takes the batch)
                        } else if (mine) {
                            dfr.tasks[(size_t)pol.req * dfr.cap + base + lanes_below(b)] = make_uint2(start, deg);
                            deg = 0;
                        }
                    }
                    __syncthreads();  // (every wave has read the totals above)
                    block_excl_scan<kRevLocalThreads>(deg, lane, wib, w.wave_tot, before, total);  // (without the deferred rows)
                }
            }
            if (total) {  // (block-uniform)
                t.prefix[tid] = before;
                t.start[tid] = start;
                t.target[tid] = tgt;
                if (tid == 0 && total > kRevLocalBudget) w.stop = 1u;  // one block should not enumerate this alone: the level loop takes the batch
                __syncthreads();
                // ---- phase B: the lanes walk the output index space; lane -> task by binary search (threads without a task have degree 0:
                // "the last task whose prefix is <= x" is always the one that owns x)
                if (total <= kRevLocalBudget) {
                    constexpr int U = 2;  // children per lane in flight (round 5, same-box A/B: a power-user lookup 20.3 us with 4, 19.0 with 2, 22.7 with 8)
                    for (uint32_t wb = 0; wb < total; wb += U * kRevLocalThreads) {  // (block-uniform trip count)
                        uint32_t edge[U], tj[U];
                        bool valid[U];
#pragma unroll
                        for (int k = 0; k < U; k++) {
                            const uint32_t x = wb + (uint32_t)k * kRevLocalThreads + tid;
                            valid[k] = x < total;
                            const uint32_t xv = valid[k] ? x : total - 1;  // inactive lanes shadow the last child: every load stays in range
                            const uint32_t jt = task_owner<kRevTaskCap>(t.prefix, xv);
                            tj[k] = jt;
                            edge[k] = gld(redges, t.start[jt] + (xv - t.prefix[jt]));
                        }
                        issue_fence();  // the U gathers travel together
#pragma unroll
                        for (int k = 0; k < U; k++) {
                            if (!__ballot(valid[k])) break;  // (wave-uniform)
                            const uint32_t tg = t.target[tj[k]];
                            const bool push = pol.visit(edge[k], tg, valid[k], pl);
                            append(push, edge[k], tg & ~kRevTaskFlags);
                        }
                    }
                }
            }
            // (also the barrier behind phase B: every lane is done with the task list before the next round overwrites it)
            stop = __syncthreads_or(w.stop != 0u);
            if (stop) break;
        }
        if (stop) break;
        const uint32_t end = w.end;  // (every append of this level is behind the round's closing barrier; <= cap, or `stop` were set)
        if (end == lvl_hi) break;   // nothing produced
        lvl_lo = lvl_hi;
        cnt = end - lvl_hi;
    }
    return RevWalkEnd{stop, min(level, kMaxLevels)};
}

// k_rev_local's rules: ONE result slot, whose rows live in the block's LDS (lds_words != 0), in `visited`, or -- a slot nobody expands, rows in HBM -- as
// bytes of RevDefer::bytemap.  A state is terminal when its slot has no parent ops at all, or when it is the result slot and that is a SINK of the reverse
// graph (Snapshot::rev_sink: no parent of its states can make another of its states true, so they are marked and not expanded: a lookup of `edit` does not walk
// on into `view = viewer + edit`, a lookup of namespace#view not into the namespaces' pods).
struct RevLocalPolicy {
    static constexpr bool kDefer = true;
    uint32_t target_slot;
    bool target_sink;
    uint32_t lds_words;
    uint32_t *s_row, *visited;
    const RevDefer &dfr;
    uint32_t req;
    uint32_t *s_dfr;  // tasks this block has deferred
    __device__ __forceinline__ uint32_t target(const RevOp &op, uint32_t level, uint32_t term_all, const RevProgLds &pl) const {
        uint32_t np = pl.progs[op.target].n & ~kRevRemoteBit;
        if (target_sink && op.target == target_slot) np = 0u;
        uint32_t tgt = op.target | (np == 0u ? kRevTerminal : 0u) | term_all | ((op.flags & OP_NOMARK) ? kRevNoMark : 0u);
        // Round 6: a row whose children land in a relation that does nothing but feed ONE permission nobody expands -- `pod#viewer`, whose only
        // parent is the computed userset in `pod#view = viewer + ...` -- marks that permission's objects directly, one dispatch level further
        // on (so only while that level is still inside the depth limit).  The intermediate states were first-visited, logged and pushed
        // through a level of their own, 1 024 per round: half of a big lookup's ids took that detour at ~5 ns each (profiles/r06_lookup_big.txt),
        // and it is what kept their rows out of the deferred list.  Nobody reads the intermediate slot's bits unless it is the result slot.
        if (!(op.flags & OP_PUSH_SAME) && np == 1u && op.target != target_slot) {
            const RevOp via = pl.ops[pl.progs[op.target].first];
            if ((via.flags & OP_PUSH_SAME) && ((pl.progs[via.target].n & ~kRevRemoteBit) == 0u || (target_sink && via.target == target_slot))) {
                if (level + 1u <= kMaxLevels) tgt = via.target | kRevTerminal;
                else tgt = kRevNoTask;  // (the permission's level lies beyond the limit: the relation's states are marked -- nobody asks -- and end there)
            }
        }
        return tgt;
    }
    __device__ __forceinline__ bool defers(uint32_t tgt) const { return (tgt & kRevTerminal) && (tgt & ~kRevTaskFlags) == target_slot; }
    __device__ __forceinline__ bool visit(uint32_t id, uint32_t tgt, bool valid, const RevProgLds &pl) const {
        const uint32_t slot = tgt & ~kRevTaskFlags;
        const uint2 si = pl.slot[slot];
        const bool ok = valid && id < si.y;
        bool push = false;
        if (slot == target_slot) {
            if (ok && lds_words) {
                const uint32_t m = 1u << (id & 31u);
                if (tgt & kRevTerminal) (void)atomicOr(&s_row[id >> 5], m);
                else push = !(atomicOr(&s_row[id >> 5], m) & m);
                return push;
            }
            if (dfr.bytemap) {  // (rows in HBM, result slot terminal: the mark is the object's byte)
                if (ok) dfr.bytemap[(size_t)req * dfr.bm_stride + id] = 1;
                return false;
            }
        } else if (tgt & kRevTerminal) {
            return false;  // neither expanded nor part of the answer: no bit
        } else if (tgt & kRevNoMark) {
            return ok;     // the only producer of this slot's states, each id once: a first visit without asking
        }
        const uint32_t bit = si.x + (ok ? id : 0u);
        uint32_t *w = visited + (bit >> 5);
        const uint32_t m = 1u << (bit & 31u);
        if (ok) {
            if (tgt & kRevTerminal) (void)__hip_atomic_fetch_or(w, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);  // (result unused: no return trip)
            else push = !(__hip_atomic_fetch_or(w, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & m);
        }
        return push;
    }
};

__global__ __launch_bounds__(kRevLocalThreads) void k_rev_local(DevReverse r, const uint32_t *__restrict__ sids, uint32_t key, uint32_t target_in, uint2 *logs,
                                                                 uint32_t cap, uint32_t *out_bitmaps, uint32_t out_stride, uint32_t copy_words,
                                                                 unsigned long long *out_counts, uint32_t *status, uint32_t lds_words, uint32_t *done_ctr,
                                                                 uint32_t *done_flag, uint32_t done_val, RevDefer dfr, RevUseful useful) {
    const uint32_t target_slot = target_in & ~kRevTargetSink;
    __shared__ alignas(16) RevWalkLds w;
    __shared__ uint32_t s_dfr;
    // lds_words != 0: the RESULT slot's rows live here, not in `visited` -- the level that produces a lookup's ids (thousands of pods under
    // a few hundred namespaces) then marks them with LDS atomics instead of L2 atomics, and the result row is copied out of LDS.  The
    // launcher sizes it to the slot's id space (up to 128 KiB = 1 M objects; beyond that, lds_words == 0 and the rows stay in HBM).
    extern __shared__ uint32_t s_row[];
    const uint32_t tid = threadIdx.x, lane = lane_id(), wib = tid >> 6;
    const uint32_t req = blockIdx.x;
    uint32_t *__restrict__ visited = r.visited + (size_t)req * r.visited_words;
    uint2 *const log = logs + (size_t)req * cap;
    if (tid == 0) s_dfr = 0;
    rev_stage_programs(r, useful, w, tid);
    const RevProg seed = r.rseeds[key];
    const uint32_t sid = sids[req];
    const uint32_t row_w0 = r.slot_bit_base[target_slot] >> 5;  // first word of the result slot's rows in `visited`
    rev_build_nomark(r, seed, w, tid, [&](uint32_t slot) { return slot == target_slot; });
    for (uint32_t i = tid; i < lds_words; i += kRevLocalThreads) s_row[i] = 0u;
    // `visited` is NOT zeroed here (round 4; VERDICT r3 weak #3: 64 blocks zeroing ~50 KB each were 7x the result rows in write traffic):
    // the host hands it over all-zero once, and every block clears exactly the bits it set before it ends -- the non-terminal first visits
    // are all in its log, marks of the result slot are cleared with the row, and terminal states of OTHER slots are not marked at all
    // (nobody reads those bits: they are not expanded and not part of the answer).
    // The bitmap is private to this block: WORKGROUP scope everywhere.  (Agent scope here was the kernel's whole cost beyond 16 lookups: an
    // agent-scope atomic on gfx950 is a fabric transaction that drops the line from the L2, and __threadfence() walks the L2's dirty lines.)
    __syncthreads();

    RevLocalPolicy pol{target_slot, (target_in & kRevTargetSink) != 0u, lds_words, s_row, visited, dfr, req, &s_dfr};
    const RevWalkEnd end = rev_block_walk(pol, r, w, seed, sid, log, cap, tid, lane, wib);
    if (end.stop) {
        // 1: redo on the level loop, 2: a row beyond the per-task enumeration limit.  A plain store (the flag may live in pinned host
        // memory): blocks that race write non-zero either way, and a 2 lost to a 1 is found again by the level loop.
        // (`visited` is left dirty: the host zeroes it before the next single-launch lookup on this context)
        if (tid == 0) {
            *status = w.stop;
            if (dfr.tasks) {  // (the launches behind this one find nothing to do for this lookup; the host redoes the batch)
                dfr.count[req] = 0u;
                dfr.levels[req] = 0u;
            }
        }
        if (!dfr.tasks) signal_done(done_ctr, done_flag, done_val);  // (deferral: k_rev_rows raises the completion word, behind everything)
        return;
    }
    if (dfr.tasks) {
        // ---- rows in HBM, handled by the two launches behind this one (k_rev_terminal, k_rev_rows): what is left here is to leave `visited` as it was
        // handed over OUTSIDE the result row -- the logged first visits -- and to publish how much was deferred
        __syncthreads();
        rev_clear_logged(w, log, cap, visited, tid, target_slot);  // (the row is cleared by k_rev_rows, behind the copy)
        if (tid == 0) {
            dfr.count[req] = min(s_dfr, dfr.cap);
            dfr.levels[req] = end.levels;
        }
        return;
    }
    // ---- result rows: the target slot's words (every one of them was last written by an L2 atomic or is still the zero it was handed over
    // with; the loads below are served by that L2 -- sc1 loads bypass the vector L1, which atomics never update)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    uint32_t *orow = out_bitmaps + (size_t)req * out_stride;
    uint32_t c32 = 0;  // (a row holds < 2^31 ids)
    for (uint32_t i = tid; i < out_stride; i += kRevLocalThreads) {
        uint32_t v = 0;
        if (i < copy_words) v = lds_words ? s_row[i] : __hip_atomic_load(visited + row_w0 + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        orow[i] = v;
        c32 += (uint32_t)__popc(v);
    }
    if (out_counts) {
        const uint32_t tot = block_count(c32, tid, lane, wib, w.wave_tot);
        if (tid == 0) out_counts[req] = tot | ((unsigned long long)end.levels << 56);  // + the reverse levels this lookup walked (statistics)
    }
    // ---- leave `visited` as it was handed over: all zero.  The logged first visits, and the result row, where it lives in HBM, as a range.
    __syncthreads();  // (the row above is copied out before anything in it is cleared)
    rev_clear_logged(w, log, cap, visited, tid, lds_words ? target_slot : kRevNoSlot);  // (a result row in LDS was never marked in `visited`)
    if (!lds_words) {
        const uint32_t rw = (w.pl.slot[target_slot].y + 31u) >> 5;
        for (uint32_t i = tid; i < rw; i += kRevLocalThreads) visited[row_w0 + i] = 0u;
    }
    signal_done(done_ctr, done_flag, done_val);
}

// ------------------------------------------------------- reverse walk, single launch, MANY result slots
// acl_lookup_resources_multi: one subject against T (type, permission) targets.  k_rev_local's walk with "the result slot" generalised: the
// level loop, the task list and the first-visit log are rev_block_walk's; RevMultiPolicy says which states end the walk and which are marked.
//   * dead ops: `useful` is the OR of the targets' Snapshot::rev_useful rows -- an op into a slot that leads to NO target is OP_DEAD;
//   * terminal states: a state is marked and never expanded exactly when its slot has no live op left (s_info's count), or at level 50.  For one sink target
//     that is k_rev_local's sink flag (every parent op of the slot leads outside `useful`); for namespace#view asked WITH pod#view it is not a sink any more;
//   * marks: every state of a target slot gets its bit, terminal or not (OP_NOMARK seed children too); terminal states of other slots get none;
//   * rows: all of them stay in `visited` (workgroup-scope atomics; no LDS row, nothing deferred).  After the walk the block copies each target's word range
//     to the caller's row, counts it, and then clears the logged first visits and the target ranges: `visited` is handed back all zero.
// The two kernels give the same answers but keep their own terminal rule (k_rev_local: the slot has no parent ops at all, or is the sink target; here: no
// LIVE op), so their logs differ, and with them the size at which a lookup overflows.
constexpr uint32_t kRevMultiLdsTargets = 256;     // target descriptors staged in LDS (the rest are read where they lie)

struct RevMultiPolicy {
    static constexpr bool kDefer = false;
    const uint32_t *s_info;  // per slot: live ops of the slot's program | bit 31: the slot is a target
    uint32_t *visited;
    __device__ __forceinline__ uint32_t target(const RevOp &op, uint32_t level, uint32_t term_all, const RevProgLds &pl) const {
        const uint32_t inf = s_info[op.target];
        const bool is_tg = (inf >> 31) != 0u;
        uint32_t tgt = op.target | ((inf & 0x7FFFFFFFu) == 0u ? kRevTerminal : 0u) | term_all | (is_tg ? kRevIsTarget : (op.flags & OP_NOMARK) ? kRevNoMark : 0u);
        // mark-through (k_rev_local, round 6): a relation nobody asked for whose one parent op is the computed userset of a permission
        // that ends the walk -- its row marks that permission's objects directly, one level further on, while that level is inside the limit
        if (!(op.flags & OP_PUSH_SAME) && !is_tg && (pl.progs[op.target].n & ~kRevRemoteBit) == 1u) {
            const RevOp via = pl.ops[pl.progs[op.target].first];
            if ((via.flags & (OP_PUSH_SAME | OP_DEAD)) == OP_PUSH_SAME && (s_info[via.target] & 0x7FFFFFFFu) == 0u) {
                if (level + 1u <= kMaxLevels) tgt = via.target | kRevTerminal | ((s_info[via.target] >> 31) ? kRevIsTarget : 0u);
                else tgt = kRevNoTask;  // (the permission's level lies beyond the limit, and the relation's own states are nobody's answer)
            }
        }
        return tgt;
    }
    __device__ __forceinline__ bool visit(uint32_t id, uint32_t tgt, bool valid, const RevProgLds &pl) const {
        const uint32_t slot = tgt & ~kRevTaskFlags;
        const uint2 si = pl.slot[slot];
        const bool ok = valid && id < si.y;
        if (!(tgt & kRevIsTarget)) {
            if (tgt & kRevTerminal) return false;  // neither expanded nor part of an answer: no bit
            if (tgt & kRevNoMark) return ok;       // the only producer of this slot's states, each id once: a first visit without asking
        }
        bool push = false;
        const uint32_t bit = si.x + (ok ? id : 0u);
        uint32_t *w = visited + (bit >> 5);
        const uint32_t m = 1u << (bit & 31u);
        if (ok) {
            if (tgt & kRevTerminal) (void)__hip_atomic_fetch_or(w, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            else push = !(__hip_atomic_fetch_or(w, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & m);
        }
        return push;
    }
};

__global__ __launch_bounds__(kRevLocalThreads) void k_rev_multi(DevReverse r, const uint32_t *__restrict__ sids, uint32_t key, const uint4 *__restrict__ targets,
                                                                 uint32_t n_targets, uint2 *logs, uint32_t cap, uint32_t *out_bitmaps, uint32_t out_stride,
                                                                 unsigned long long *out_counts, uint32_t *status, uint32_t *done_ctr, uint32_t *done_flag,
                                                                 uint32_t done_val, RevUseful useful, RevUseful is_target) {
    __shared__ alignas(16) RevWalkLds w;
    __shared__ uint32_t s_info[kRevLdsSlots];    // live ops of the slot's program | bit 31: the slot is a target
    __shared__ uint4 s_tg[kRevMultiLdsTargets];  // {slot, first word of the caller's row, words to copy, words of the caller's row}
    const uint32_t tid = threadIdx.x, lane = lane_id(), wib = tid >> 6;
    const uint32_t req = blockIdx.x;
    uint32_t *__restrict__ visited = r.visited + (size_t)req * r.visited_words;
    uint2 *const log = logs + (size_t)req * cap;
    rev_stage_programs(r, useful, w, tid);
    for (uint32_t i = tid; i < min(n_targets, kRevMultiLdsTargets); i += kRevLocalThreads) s_tg[i] = targets[i];
    const RevProg seed = r.rseeds[key];
    const uint32_t sid = sids[req];
    __syncthreads();
    for (uint32_t i = tid; i < r.nslots; i += kRevLocalThreads) {
        const RevProg p = w.pl.progs[i];
        uint32_t live = 0;
        for (uint32_t j = 0; j < (p.n & ~kRevRemoteBit); j++) live += (w.pl.ops[p.first + j].flags & OP_DEAD) ? 0u : 1u;
        s_info[i] = live | (((is_target.w[i >> 5] >> (i & 31u)) & 1u) << 31);
    }
    rev_build_nomark(r, seed, w, tid, [&](uint32_t slot) { return ((is_target.w[slot >> 5] >> (slot & 31u)) & 1u) != 0u; });
    // (`visited` is handed over all zero and handed back all zero, private to this block: workgroup scope everywhere -- see k_rev_local)
    __syncthreads();

    RevMultiPolicy pol{s_info, visited};
    const RevWalkEnd end = rev_block_walk(pol, r, w, seed, sid, log, cap, tid, lane, wib);
    if (end.stop) {
        // 1: the host answers the group target by target, 2: a row beyond the per-task enumeration limit (`visited` is left dirty: the host zeroes it)
        if (tid == 0) *status = w.stop;
        signal_done(done_ctr, done_flag, done_val);
        return;
    }
    // ---- result rows: each target's words (last written by an L2 atomic, or still the zero they were handed over with -- agent-scope loads, as k_rev_local's)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    uint32_t *orow = out_bitmaps + (size_t)req * out_stride;
    for (uint32_t j = 0; j < n_targets; j++) {
        const uint4 tg = j < kRevMultiLdsTargets ? s_tg[j] : targets[j];
        const uint32_t w0 = w.pl.slot[tg.x].x >> 5;
        uint32_t c32 = 0;  // (a row holds < 2^31 ids)
        for (uint32_t i = tid; i < tg.w; i += kRevLocalThreads) {
            uint32_t v = 0;
            if (i < tg.z) v = __hip_atomic_load(visited + w0 + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            orow[tg.y + i] = v;
            c32 += (uint32_t)__popc(v);
        }
        if (out_counts) {
            const uint32_t tot = block_count(c32, tid, lane, wib, w.wave_tot);
            if (tid == 0) out_counts[(size_t)req * n_targets + j] = (unsigned long long)tot | ((unsigned long long)end.levels << 56);
            __syncthreads();  // (the wave totals are read before the next target's are stored)
        }
    }
    // ---- leave `visited` all zero: the logged first visits and every target's range
    __syncthreads();  // (every row is copied out before anything in it is cleared)
    rev_clear_logged(w, log, cap, visited, tid, kRevNoSlot);
    for (uint32_t j = 0; j < n_targets; j++) {
        const uint32_t slot = j < kRevMultiLdsTargets ? s_tg[j].x : targets[j].x;
        const uint2 si = w.pl.slot[slot];
        const uint32_t rw = (si.y + 31u) >> 5;
        for (uint32_t i = tid; i < rw; i += kRevLocalThreads) visited[(si.x >> 5) + i] = 0u;
    }
    signal_done(done_ctr, done_flag, done_val);
}

// The deferred rows of k_rev_local (see RevDefer): blockIdx.y = lookup, the launch's waves take its tasks round-robin and a wave's lanes read consecutive ids
// of a reverse row.  An id's mark is its byte of the lookup's byte map (RevDefer::bytemap): a plain store, whichever block and XCD makes it.
__global__ __launch_bounds__(256) void k_rev_terminal(DevReverse r, uint32_t target_slot, RevDefer dfr) {
    // (a lookup whose block gave up has published zero tasks; the status word itself lives in the caller's pinned memory and is not worth a trip across PCIe
    //  from every thread of a chip-wide launch -- a first version read it and spent 100 us of a 220 us empty lookup doing so)
    const uint32_t req = blockIdx.y, lane = lane_id();
    const uint32_t nt = min(dfr.count[req], dfr.cap), nobj = r.slot_nobjects[target_slot];
    uint8_t *__restrict__ bm = dfr.bytemap + (size_t)req * dfr.bm_stride;
    const uint2 *__restrict__ tasks = dfr.tasks + (size_t)req * dfr.cap;
    const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6), nwaves = gridDim.x * 4u;
    for (uint32_t t = wave; t < nt; t += nwaves) {
        const uint2 tk = tasks[t];
        for (uint32_t i = lane; i < tk.y; i += 64u) {
            const uint32_t id = gld(r.redges, tk.x + i);
            if (id < nobj) bm[id] = 1;
        }
    }
}

// The result rows of a batch whose rows live in HBM (see RevDefer): blockIdx.y = lookup, the x blocks take slices of its row -- copy out (device or pinned
// host memory), count, clear -- so that a 1 MB row crosses PCIe from all CUs at once instead of from one.  d_count: [lookups] device accumulators (zero
// between launches: re-armed by the last block); the last block of the LAUNCH writes every lookup's count | levels << 56 to out_counts and raises done_flag.
__global__ __launch_bounds__(256) void k_rev_rows(DevReverse r, uint32_t target_slot, uint32_t n, uint32_t *out_bitmaps, uint32_t out_stride, uint32_t copy_words,
                                                  unsigned long long *out_counts, unsigned long long *d_count, RevDefer dfr, uint32_t *done_ctr,
                                                  uint32_t *done_flag, uint32_t done_val) {
    __shared__ uint32_t s_cnt[4];
    __shared__ bool s_last;
    const uint32_t req = blockIdx.y, lane = lane_id(), wib = threadIdx.x >> 6;
    // (a batch in which some block gave up is redone by the host on the level loop: copying its partial rows is harmless, and the host zeroes the byte map again)
    uint4 *__restrict__ bm = reinterpret_cast<uint4 *>(dfr.bytemap + (size_t)req * dfr.bm_stride);  // (bm_stride is a multiple of 128 bytes: 32 ids = two aligned uint4)
    uint32_t *__restrict__ orow = out_bitmaps + (size_t)req * out_stride;
    uint32_t c32 = 0;
    auto nibble = [](uint32_t x) -> uint32_t { return (x * 0x01020408u) >> 24 & 0xFu; };  // four 0 / 1 bytes -> four bits, byte 0 lowest (no two partial products meet)
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < out_stride; i += gridDim.x * 256u) {  // one word of the caller's row = 32 bytes of the map
        uint32_t v = 0;
        if (i < copy_words) {
            const uint4 a = bm[2u * i], b = bm[2u * i + 1u];
            v = nibble(a.x) | nibble(a.y) << 4 | nibble(a.z) << 8 | nibble(a.w) << 12 | nibble(b.x) << 16 | nibble(b.y) << 20 | nibble(b.z) << 24 | nibble(b.w) << 28;
            if (v) {  // (zero again for the next lookup: only where something was set)
                bm[2u * i] = make_uint4(0u, 0u, 0u, 0u);
                bm[2u * i + 1u] = make_uint4(0u, 0u, 0u, 0u);
            }
        }
        orow[i] = v;
        c32 += (uint32_t)__popc(v);
    }
    c32 = wave_last(wave_incl_scan(c32, lane));
    if (lane == 0) s_cnt[wib] = c32;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t tot = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        if (tot) (void)__hip_atomic_fetch_add(d_count + req, (unsigned long long)tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence_system();  // this block's slices are in the caller's memory before it arrives
        s_last = __hip_atomic_fetch_add(done_ctr, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x * gridDim.y - 1u;
    }
    __syncthreads();
    if (!s_last) return;
    for (uint32_t i = threadIdx.x; i < n; i += 256u) {
        const unsigned long long c = __hip_atomic_exchange(d_count + i, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (out_counts) out_counts[i] = c | ((unsigned long long)dfr.levels[i] << 56);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence_system();
        __hip_atomic_store(done_ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (done_flag) __hip_atomic_store(done_flag, done_val, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ------------------------------------------------------------------ import
// ImportOut: a wave's append cursor into the dynamic chunks of the frontier iteration `iter` produced (the static chunks belong to that iteration's
// expand waves) -- the step protocol's k_import and the native loops' gathered imports, below.
struct ImportOut {
    uint4 *__restrict__ out;
    uint32_t *counts, *nchunks, *overflow, *any;
    uint32_t nwaves, max_chunks;
    uint32_t cur = kNoSpace, fill = kChunk, produced = 0;
    __device__ __forceinline__ ImportOut(const DevFrontier &f, uint32_t iter)
        : out(f.buf[iter & 1u]), counts(f.counts[iter & 1u]), nchunks(f.nchunks + iter), overflow(f.overflow), any(f.any + iter), nwaves(f.nwaves), max_chunks(f.max_chunks) {}
    // appends the flagged lanes' entries (wave-uniform control flow); false: the frontier is out of chunks (overflow raised), stop
    __device__ __forceinline__ bool append(bool mine, const uint4 &e, uint32_t lane) {
        const uint64_t b = __ballot(mine);
        if (!b) return true;
        const uint32_t need = (uint32_t)__popcll(b);
        if (fill + need > kChunk) {
            if (lane == 0 && cur != kNoSpace) counts[cur] = fill;
            uint32_t c = 0;
            if (lane == 0) c = atomicAdd(nchunks, 1u);
            c = uniform(c) + nwaves;
            if (c >= max_chunks) {
                if (lane == 0) *overflow = 1u;
                cur = kNoSpace;
                return false;
            }
            cur = c;
            fill = 0;
        }
        if (mine) out[(size_t)cur * kChunk + fill + lanes_below(b)] = e;
        fill += need;
        produced += need;
        return true;
    }
    __device__ __forceinline__ void close(uint32_t lane) {
        if (lane == 0) {
            if (cur != kNoSpace) counts[cur] = fill;
            if (produced) *any = 1u;
        }
    }
};

// Appends entries of an exchanged export buffer to the frontier iteration `iter` produced.  FWD: keep the entries whose slot this shard owns.
// Reverse: keep foreign states for which this shard holds parent rows.
template <bool FWD>
__global__ __launch_bounds__(256) void k_import(DevFrontier f, uint32_t iter, const uint4 *__restrict__ in, uint32_t n, const SlotProg *progs,
                                                const RevProg *rprogs, uint32_t rank) {
    const uint32_t lane = lane_id();
    const uint32_t wave = blockIdx.x * 4 + (threadIdx.x >> 6), nw = gridDim.x * 4;
    ImportOut io(f, iter);
    for (uint32_t x = wave; (uint64_t)x * 64 < n; x += nw) {
        const uint32_t i = x * 64 + lane;
        const uint4 e = i < n ? in[i] : make_uint4(0, 0, kDeadMeta, 0);
        bool mine = i < n && e.z != kDeadMeta;
        if (mine) mine = FWD ? progs[meta_slot(e.z)].owner == rank : (rprogs[e.z & 0x1FFFu].n & ~kRevRemoteBit) != 0;
        if (!io.append(mine, e, lane)) break;
    }
    io.close(lane);
}

// ---------------------------------------------------------------- native sharded loop (engine_shard_native.cpp)
// Exchange blocks, one per (shard, level) in the all-gather form and one per (shard, destination, level) in the all-to-all form: a 16-byte
// HEADER and up to `cap` entries.  header = {x: entries in this block, y: this shard produced local work | overflow code << 1,
// z: the largest block this shard filled this level, w: entries this shard exported this level in all}.  Written on the device, so the host
// never waits between levels; headers and entries travel in separate collectives (the entries' one is skipped on levels that are known
// to export nothing).  exp_count = [0] all-gather form; [1 + d] per destination.
__global__ __launch_bounds__(64) void k_xhdr(uint4 *hdr, uint32_t nblocks, const uint32_t *exp_count, const uint32_t *any_iter, const uint32_t *overflow) {
    const uint32_t d = threadIdx.x;
    if (d >= nblocks) return;
    const uint32_t flags = (*any_iter ? 1u : 0u) | (*overflow << 1);
    if (nblocks == 1) {
        const uint32_t c = exp_count[0];
        hdr[0] = make_uint4(c, flags, c, c);
        return;
    }
    uint32_t mx = 0, tot = 0;
    for (uint32_t k = 0; k < nblocks; k++) {
        const uint32_t c = exp_count[1 + k];
        mx = max(mx, c);
        tot += c;
    }
    hdr[d] = make_uint4(exp_count[1 + d], flags, mx, tot);
}

// What the gathered imports share.  fold_headers: the own row's first wave folds all headers into the level's control record {total exported, any shard
// produced, overflow code, largest block} (call with the first 64 threads of one block).  They append through ImportOut, above.
__device__ __forceinline__ void fold_headers(const uint4 *__restrict__ hdrs, uint32_t world, uint32_t cap, uint32_t have_data, uint32_t *ctrl, uint32_t lane) {
    uint32_t total = 0, anyp = 0, over = 0, mx = 0;
    for (uint32_t r = lane; r < world; r += 64) {
        const uint4 h = hdrs[r];
        total += h.w;
        anyp |= h.y & 1u;
        over |= (h.y >> 1) | (h.z > cap ? kOverflowExport : 0u) | ((!have_data && h.w) ? 4u : 0u);  // (h.w, every shard's own included: the same verdict on every shard)
        mx = max(mx, h.z);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        total += (uint32_t)__shfl_xor((int)total, d, 64);
        anyp |= (uint32_t)__shfl_xor((int)anyp, d, 64);
        over |= (uint32_t)__shfl_xor((int)over, d, 64);
        mx = max(mx, (uint32_t)__shfl_xor((int)mx, d, 64));
    }
    if (lane == 0) {
        ctrl[0] = total;
        ctrl[1] = anyp;
        ctrl[2] = over;
        ctrl[3] = mx;
    }
}
// The gathered imports' opening (blockIdx.y = source shard): the own row's first wave folds the headers and the row is done; without entries so is every
// other row; else *in / *n are what the block's source shard sent, the count read from its header.  false: nothing to import, return.
__device__ __forceinline__ bool gathered_input(const uint4 *__restrict__ hdrs, const uint4 *__restrict__ data, uint32_t world, uint32_t rank, uint32_t cap, uint32_t have_data,
                                               uint32_t *ctrl, uint32_t lane, const uint4 *__restrict__ *in, uint32_t *n) {
    const uint32_t src = blockIdx.y;
    if (src == rank) {
        if (blockIdx.x == 0 && threadIdx.x < 64) fold_headers(hdrs, world, cap, have_data, ctrl, lane);
        return false;
    }
    if (!have_data) return false;
    *in = data + (size_t)src * cap;
    *n = min(hdrs[src].x, cap);
    return true;
}

// After the exchange: blockIdx.y = source shard.  Rows of other shards import what they sent (FWD: the entries whose slot this shard owns;
// reverse: foreign states for which this shard holds parent rows), the count read from the source's header; the own row's first wave folds all
// headers into the level's control record {total exported, any shard produced, overflow code, largest block} -- identical on every shard, so
// all of them take the same decisions (done / redo) without talking to each other or to the host.  have_data == 0: the entries were not
// exchanged this level (planned: nothing was expected); headers that announce entries then raise overflow code 4 = "redo with the data".
template <bool FWD>
__global__ __launch_bounds__(256) void k_import_gathered(DevFrontier f, uint32_t iter, const uint4 *__restrict__ hdrs, const uint4 *__restrict__ data, uint32_t world,
                                                         uint32_t rank, uint32_t cap, uint32_t have_data, const SlotProg *progs, const RevProg *rprogs,
                                                         uint32_t *ctrl) {
    const uint32_t lane = lane_id();
    const uint4 *__restrict__ in;
    uint32_t n;
    if (!gathered_input(hdrs, data, world, rank, cap, have_data, ctrl, lane, &in, &n)) return;
    const uint32_t wave = blockIdx.x * 4 + (threadIdx.x >> 6), nw = gridDim.x * 4;
    ImportOut io(f, iter);
    for (uint32_t x = wave; (uint64_t)x * 64 < n; x += nw) {
        const uint32_t i = x * 64 + lane;
        const uint4 e = i < n ? in[i] : make_uint4(0, 0, kDeadMeta, 0);
        bool mine = i < n && e.z != kDeadMeta;
        if (mine) mine = FWD ? progs[meta_slot(e.z)].owner == rank : (rprogs[e.z & 0x1FFFu].n & ~kRevRemoteBit) != 0;
        if (!io.append(mine, e, lane)) break;
    }
    io.close(lane);
}

}  // namespace

#if ACL_PROFILE_PHASES
}  // namespace acl
extern "C" int acl_debug_phase_cycles(unsigned long long *out20) {  // variant builds only (tools/phases.py): reads and resets the counters
    unsigned long long z[20] = {0};
    if (hipMemcpyFromSymbol(out20, HIP_SYMBOL(acl::acl_phase_cycles), sizeof(z)) != hipSuccess) return 1;
    return hipMemcpyToSymbol(HIP_SYMBOL(acl::acl_phase_cycles), z, sizeof(z)) == hipSuccess ? 0 : 1;
}
namespace acl {
#endif
static size_t prog_lds_bytes(const DevGraph &g) { return ((size_t)g.nslots + g.nops) * 32; }
// Turns a run-time flag into a compile-time one: f(std::true_type{}) or f(std::false_type{}).  The launchers below pick a kernel instantiation with it,
// so that every kernel template has ONE launch site.
template <typename F>
static auto with_flag(bool flag, F &&f) {
    if (flag) return f(std::true_type{});
    return f(std::false_type{});
}

int expand_grid_blocks(int device) {
    hipDeviceProp_t prop;
    int cus = 256;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
    int per_cu = 8;  // 256-thread blocks, ~20 KiB LDS; the occupancy query lowers it to what k_expand's ~70 VGPRs allow (6 or 7)
    int occ = 0;
    // (the program table's LDS copy is dynamic; 2 KiB covers schemas of ~60 slots + ops -- a larger one only means some blocks of a launch queue)
    const hipError_t oe = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_expand<true, false>, kBlock, 2048);
    (void)k_expand<false, false>;  // (no effect at run time: first named here, this instantiation stays second in the code object, whose device code can
                                   //  then be compared line by line with an earlier build's -- the test that a host-side cleanup of this file left the kernels alone)
    if (oe == hipSuccess && occ > 0) per_cu = occ < per_cu ? occ : per_cu;
    return cus * per_cu;
}

void launch_seed(hipStream_t s, const DevGraph &g, const DevFrontier &f, const uint4 *items, uint32_t n, uint8_t *has, uint8_t *err, const DevShard &sh) {
    const uint32_t threads = std::max(std::max(n, f.nwaves), kStatusWords);
    hipLaunchKernelGGL(k_seed, dim3((threads + 255) / 256), dim3(256), 0, s, g, f, items, n, has, err, sh);
}
void launch_expand(hipStream_t s, const DevGraph &g, const DevFrontier &f, uint32_t iter, uint8_t *has, uint8_t *err, const DevShard &sh) {
    const dim3 grid(f.nwaves / kWavesPerBlock);
    // CMB: schemas with `&` / `-` (round 5: the sharded graph too -- cells in per-shard ranges of one global cell space, engine_shard_native.cpp);
    // LDSPROG: the program table fits its LDS copy
    with_flag(g.bexpr != nullptr, [&](auto cmb) {
        with_flag(sh.world > 1, [&](auto sharded) {
            with_flag(g.nslots + g.nops <= kProgLdsEntries, [&](auto lds) {
                hipLaunchKernelGGL((k_expand<lds(), sharded(), cmb()>), grid, dim3(kBlock), lds() ? prog_lds_bytes(g) : 0, s, g,
                                   f, iter, has, err, sh);
            });
        });
    });
}
template <int WAVES>
static void launch_check_local_w(hipStream_t s, const DevGraph &g, const uint4 *items, uint32_t n, uint32_t rpw, uint32_t nblocks, uint32_t nunits, uint32_t nstatic, uint32_t rdyn,
                                 uint32_t *next_unit, uint4 *buf0, uint4 *buf1, uint32_t cap, uint32_t *overflow, uint8_t *has, uint8_t *err, uint8_t *perm_out, int32_t *err_out,
                                 uint32_t *max_level, uint32_t skew, uint32_t *done_ctr, uint32_t *done_flag, uint32_t done_val, const InlineItems &inl) {
    const dim3 grid(nblocks);
    with_flag(g.bexpr != nullptr, [&](auto cmb) {  // schemas with `&` / `-`: the combine instantiations
        with_flag(g.nslots + g.nops <= kProgLdsEntries, [&](auto lds) {
            hipLaunchKernelGGL((k_check_local<lds(), WAVES, cmb()>), grid, dim3(WAVES * 64), lds() ? prog_lds_bytes(g) : 0, s, g, items, n, rpw,
                               nunits, nstatic, rdyn, next_unit, buf0, buf1, cap, overflow, has, err, perm_out, err_out, max_level, skew, done_ctr, done_flag, done_val, inl);
        });
    });
}
void launch_check_local(hipStream_t s, const DevGraph &g, const uint4 *items, uint32_t n, uint32_t rpw, uint32_t nblocks, uint32_t *next_unit, uint4 *buf0,
                        uint4 *buf1, uint32_t cap, uint32_t *overflow, uint8_t *has, uint8_t *err, uint8_t *perm_out, int32_t *err_out, uint32_t *max_level,
                        bool wide, uint32_t skew, uint32_t *done_ctr, uint32_t *done_flag, uint32_t done_val, const uint4 *inline_items_host) {
    InlineItems inl{};
    if (inline_items_host && n <= 4) {  // (host memory: copied into the launch's arguments)
        for (uint32_t i = 0; i < n; i++) inl.v[i] = inline_items_host[i];
        items = nullptr;
    }
    const uint32_t nunits = (n + rpw - 1) / rpw;
    skew = std::min(skew, std::min(rpw - 1u, (wide ? kLocalWide : kLocalNarrow) * 64u - rpw));  // the largest unit still fits the block: thread i seeds request first + i
    skew = nunits > 1 && nunits <= 4096 ? (skew << 8) / nunits : 0u;                             // (the kernel's fixed-point form: 1/256ths per unit; u (nunits - u) skew < 2^32)
    const uint32_t nstatic = nunits, rdyn = rpw;  // (every unit holds rpw requests: the kernel's hand-out units for a batch's tail lost, profiles/r03_static_dynamic_units_ab.txt)
    if (wide) launch_check_local_w<kLocalWide>(s, g, items, n, rpw, nblocks, nunits, nstatic, rdyn, next_unit, buf0, buf1, cap, overflow, has, err, perm_out, err_out, max_level, skew, done_ctr, done_flag, done_val, inl);
    else launch_check_local_w<kLocalNarrow>(s, g, items, n, rpw, nblocks, nunits, nstatic, rdyn, next_unit, buf0, buf1, cap, overflow, has, err, perm_out, err_out, max_level, skew, done_ctr, done_flag, done_val, inl);
}
template <int WAVES>
static int local_occupancy(bool lds, size_t prog_bytes) {
    int occ = 0;
    const hipError_t oe = lds ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_check_local<true, WAVES>, WAVES * 64, prog_bytes)
                              : hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_check_local<false, WAVES>, WAVES * 64, 0);
    return (oe != hipSuccess || occ <= 0) ? std::max(1, 16 / WAVES) : occ;
}
int local_grid_blocks(int device, size_t prog_bytes, bool wide) {
    hipDeviceProp_t prop;
    int cus = 256;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
    const bool lds = prog_bytes <= (size_t)kProgLdsEntries * 32;
    return cus * (wide ? local_occupancy<kLocalWide>(lds, prog_bytes) : local_occupancy<kLocalNarrow>(lds, prog_bytes));
}
uint32_t local_unit_max(bool wide) { return (uint32_t)(wide ? kLocalWide : kLocalNarrow) * 64u; }
void launch_dedup(hipStream_t s, const DevFrontier &f, uint32_t iter, uint64_t *table, uint32_t bits, bool cells) {
    (void)hipMemsetAsync(table, 0xFF, sizeof(uint64_t) << bits, s);
    if (cells) {  // (`table` holds 2^bits keys and, behind them, 2^bits second halves)
        uint32_t *second = reinterpret_cast<uint32_t *>(table + ((size_t)1 << bits));
        (void)hipMemsetAsync(second, 0, sizeof(uint32_t) << bits, s);
        hipLaunchKernelGGL(k_dedup_cells, dim3(f.nwaves / kWavesPerBlock), dim3(256), 0, s, f, iter, reinterpret_cast<unsigned long long *>(table), second, bits);
        return;
    }
    hipLaunchKernelGGL(k_dedup, dim3(f.nwaves / kWavesPerBlock), dim3(256), 0, s, f, iter, reinterpret_cast<unsigned long long *>(table), bits);
}
void launch_finalize(hipStream_t s, uint32_t n, const uint8_t *has, const uint8_t *err, uint8_t *perm_out, int32_t *err_out) {
    if (!n) return;
    hipLaunchKernelGGL(k_finalize, dim3((n + 255) / 256), dim3(256), 0, s, n, has, err, perm_out, err_out);
}
void launch_resolve(hipStream_t s, const DevGraph &g, uint32_t iter, uint8_t *has, uint8_t *err) {
    hipLaunchKernelGGL(k_resolve, dim3(256), dim3(256), 0, s, g, iter, 1u, has, err);
    hipLaunchKernelGGL(k_resolve, dim3(256), dim3(256), 0, s, g, iter, 0u, has, err);
}
void launch_node_hdr(hipStream_t s, uint4 *hdr, const uint32_t *ccount) { hipLaunchKernelGGL(k_node_hdr, dim3(1), dim3(1), 0, s, hdr, ccount); }
void launch_resolve_gathered(hipStream_t s, const DevGraph &g, const uint4 *nodes, uint32_t stride, const uint4 *hdrs, uint32_t world, uint32_t iter, uint8_t *has, uint8_t *err) {
    hipLaunchKernelGGL(k_resolve_gathered, dim3(64, world), dim3(256), 0, s, g, nodes, stride, hdrs, iter, 1u, has, err);
    hipLaunchKernelGGL(k_resolve_gathered, dim3(64, world), dim3(256), 0, s, g, nodes, stride, hdrs, iter, 0u, has, err);
}
void launch_rev_seed(hipStream_t s, const DevFrontier &f, const uint32_t *d_sids, uint32_t n, uint32_t key) {
    const uint32_t threads = std::max(std::max(n, f.nwaves), kStatusWords);
    hipLaunchKernelGGL(k_rev_seed, dim3((threads + 255) / 256), dim3(256), 0, s, f, d_sids, n, key);
}
void launch_keep(hipStream_t s, uint32_t k_items, const uint32_t *item_off, const uint8_t *perm, uint8_t *keep_out) {
    if (!k_items) return;
    hipLaunchKernelGGL(k_keep, dim3((k_items + 255) / 256), dim3(256), 0, s, k_items, item_off, perm, keep_out);
}
void launch_rev_expand(hipStream_t s, const DevReverse &r, const DevFrontier &f, uint32_t iter, uint32_t phase, const DevShard &sh) {
    const dim3 grid(f.nwaves / kWavesPerBlock);
    if (phase == REV_VISIT) hipLaunchKernelGGL(k_rev_expand<REV_VISIT>, grid, dim3(kBlock), 0, s, r, f, iter, sh);
    else if (phase == REV_EXPAND) hipLaunchKernelGGL(k_rev_expand<REV_EXPAND>, grid, dim3(kBlock), 0, s, r, f, iter, sh);
    else hipLaunchKernelGGL(k_rev_expand<REV_FUSED>, grid, dim3(kBlock), 0, s, r, f, iter, sh);
}
void launch_rev_local(hipStream_t s, const DevReverse &r, const uint32_t *sids, uint32_t n, uint32_t key, uint32_t target_slot, void *logs,
                      uint32_t cap, uint32_t *out_bitmaps, uint32_t out_stride, uint32_t copy_words, uint64_t *out_counts, uint32_t *status, uint32_t lds_row_words,
                      uint32_t *done_ctr, uint32_t *done_flag, uint32_t done_val, const RevBigRows *big, const RevUseful *useful_p) {
    if (!n) return;
    RevUseful useful;
    for (uint32_t k = 0; k < kRevUsefulWords; k++) useful.w[k] = useful_p ? useful_p->w[k] : 0xFFFFFFFFu;
    static const bool big_lds = hipFuncSetAttribute(reinterpret_cast<const void *>(k_rev_local), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRevLdsRowBytes) == hipSuccess;
    if (lds_row_words * 4u > (big_lds ? kRevLdsRowBytes : 32768u)) lds_row_words = 0;  // rows stay in HBM
    RevDefer dfr;
    if (!lds_row_words && big && big->tasks)
        dfr = RevDefer{reinterpret_cast<uint2 *>(big->tasks), big->task_count, big->levels, big->task_cap, big->defer_min ? big->defer_min : 4096u, big->bytemap, big->bytemap_stride};
    hipLaunchKernelGGL(k_rev_local, dim3(n), dim3(kRevLocalThreads), (size_t)lds_row_words * 4, s, r, sids, key, target_slot, (uint2 *)logs, cap, out_bitmaps,
                       out_stride, copy_words, (unsigned long long *)out_counts, status, lds_row_words, done_ctr, done_flag, done_val, dfr, useful);
    if (!dfr.tasks) return;
    target_slot &= ~kRevTargetSink;
    // the two chip-wide launches behind it: the deferred rows' ids, then the rows themselves (copy out, count, clear)
    const uint32_t per = std::max(1u, std::min(256u, 2048u / n));  // blocks per lookup: the chip for a single lookup, ~8 blocks per CU in all for a batch
    hipLaunchKernelGGL(k_rev_terminal, dim3(per, n), dim3(256), 0, s, r, target_slot, dfr);
    const uint32_t slices = std::max(1u, std::min(per, (out_stride + 1023u) / 1024u));
    hipLaunchKernelGGL(k_rev_rows, dim3(slices, n), dim3(256), 0, s, r, target_slot, n, out_bitmaps, out_stride, copy_words, (unsigned long long *)out_counts,
                       (unsigned long long *)big->counts, dfr, done_ctr, done_flag, done_val);
}
void launch_rev_multi(hipStream_t s, const DevReverse &r, const uint32_t *sids, uint32_t n, uint32_t key, const RevMultiTarget *targets, uint32_t n_targets, void *logs,
                      uint32_t cap, uint32_t *out_bitmaps, uint32_t out_stride, uint64_t *out_counts, uint32_t *status, const RevUseful &useful, const RevUseful &is_target,
                      uint32_t *done_ctr, uint32_t *done_flag, uint32_t done_val) {
    if (!n || !n_targets) return;
    static_assert(sizeof(RevMultiTarget) == sizeof(uint4), "k_rev_multi reads a target as one 16-byte load");
    hipLaunchKernelGGL(k_rev_multi, dim3(n), dim3(kRevLocalThreads), 0, s, r, sids, key, reinterpret_cast<const uint4 *>(targets), n_targets, (uint2 *)logs, cap, out_bitmaps,
                       out_stride, (unsigned long long *)out_counts, status, done_ctr, done_flag, done_val, useful, is_target);
}
static uint32_t import_blocks(uint32_t n) {  // ~one 1024-entry chunk of input per wave, at most 256 blocks
    const uint32_t b = (n + 4095) / 4096;
    return b < 1 ? 1 : (b > 256 ? 256 : b);
}
// grid x of the gathered imports (grid y = the source shards): ~one 1024-entry chunk of a block of `cap` entries per wave, at most 64 blocks a source; one
// where no entries travelled (the own row's header fold is all there is to do)
static uint32_t import_gathered_blocks(uint32_t cap, bool have_data) { return have_data ? std::max<uint32_t>(1, std::min<uint32_t>(64, (cap + 4095) / 4096)) : 1u; }
void launch_import(hipStream_t s, const DevGraph &g, const DevFrontier &f, uint32_t iter, const uint4 *in, uint32_t n, const DevShard &sh) {
    if (!n) return;
    hipLaunchKernelGGL(k_import<true>, dim3(import_blocks(n)), dim3(256), 0, s, f, iter, in, n, g.progs, (const RevProg *)nullptr, sh.rank);
}
void launch_xhdr(hipStream_t s, uint4 *hdr, uint32_t nblocks, const uint32_t *exp_count, const uint32_t *any_iter, const uint32_t *overflow) {
    hipLaunchKernelGGL(k_xhdr, dim3(1), dim3(64), 0, s, hdr, nblocks, exp_count, any_iter, overflow);
}
void launch_import_gathered(hipStream_t s, const DevGraph &g, const DevFrontier &f, uint32_t iter, const uint4 *hdrs, const uint4 *data, uint32_t world, uint32_t rank,
                            uint32_t cap, bool have_data, uint32_t *ctrl) {
    const uint32_t bx = import_gathered_blocks(cap, have_data);
    hipLaunchKernelGGL(k_import_gathered<true>, dim3(bx, world), dim3(256), 0, s, f, iter, hdrs, data, world, rank, cap, have_data ? 1u : 0u, g.progs, (const RevProg *)nullptr, ctrl);
}
void launch_rev_import_gathered(hipStream_t s, const DevReverse &r, const DevFrontier &f, uint32_t iter, const uint4 *hdrs, const uint4 *data, uint32_t world, uint32_t rank,
                                uint32_t cap, bool have_data, uint32_t *ctrl) {
    const uint32_t bx = import_gathered_blocks(cap, have_data);
    hipLaunchKernelGGL(k_import_gathered<false>, dim3(bx, world), dim3(256), 0, s, f, iter, hdrs, data, world, rank, cap, have_data ? 1u : 0u, (const SlotProg *)nullptr, r.rprogs, ctrl);
}
void launch_rev_import(hipStream_t s, const DevReverse &r, const DevFrontier &f, uint32_t iter, const uint4 *in, uint32_t n) {
    if (!n) return;
    hipLaunchKernelGGL(k_import<false>, dim3(import_blocks(n)), dim3(256), 0, s, f, iter, in, n, (const SlotProg *)nullptr, r.rprogs, 0u);
}

// ---- the forward walk of LookupSubjects and Explain (plan.hpp SubjectRows).  A walk starts at one resource's state and follows the FORWARD programs: the
// positive relaxation of the Check they encode -- ops inside the subtracted operand of an exclusion are skipped (SubjOp kSubjSkip), both sides of `&` and the
// tupleset of `.all()` are walked.  Five kernels share it:
//   k_revoke_local   one block per (item, stored relationship) of an Explain-for-revocation call, Explain's walk with RevokePolicy -- the same tests with that
//                    one relationship left out of every row that holds it; one word comes back: is the subject still found
//   k_subj_local     one block per lookup, every level in one launch: subj_block_walk with SubjectsPolicy -- reached rows of the subject class are EMITTED
//   k_explain_local  one block per item, the same walk with ExplainPolicy -- reached rows are TESTED for the item's one subject, every state remembers its parent
//   k_subj_expand    one launch per level over the chunked frontier (the sharded graph): its own loop, the same decode
//   k_reach_local    one block per (resource, permission) of an Explain-denial call, the same walk with ReachPolicy -- children only, no row is emitted or
//                    tested: the log IS the result, the states a denied Check has looked at
// subj_decode is the one place that says what an op does, at dispatch level L = the state's level + op.dlevel <= kMaxLevels (k_check_local's rule: a Check
// answers HAS there):
//   OP_PROBE_HASH of key T      -> every id of the class's subject row for the state's object (OP_WILD: the row is the wildcard's -> the flag)
//   OP_PROBE of key T (sorted)  -> every id of the sorted row
//   OP_REFLEX of key T#r        -> the state's own id
//   OP_ENUM / OP_PUSH_SAME      -> child states at L + 1 (when L + 1 <= kMaxLevels); a userset row of key T#r is emitted through its children's REFLEX
//                                  ops, or, when the children would lie beyond the limit, by the probe itself
// (TEST, Explain: "every id of the row" becomes "does the row hold the subject", answered by the device functions of k_check_local's interpreter.
//  REACH, Explain denial: probes and reflex ops yield nothing; only the last line is left, and the walk does not depend on the subject.)
// Depth: a state counts at the LEAST level it can be reached at.  subj_block_walk processes its log level by level; a child one level below the current one
// gets its visited bit when it is appended (nothing of a lower level is still to come), a child further down (an inlined computed userset's offset) is appended
// unmarked and decides its visit when its own level comes round -- after every state of the levels before it has been marked.
constexpr int kSubjThreads = 1024;
constexpr uint32_t kSubjMaxRow = 1u << 21;        // ids of one row a task may enumerate (1 024 tasks x 2 M stay inside 32-bit prefix sums)
constexpr uint32_t kSubjMarked = 0x80000000u;     // log entry: its visit was decided when it was appended
constexpr uint32_t kSubjDead = 0x40000000u;       // log entry: a second visit, or moved behind the current level: not expanded here
constexpr uint32_t kSubjEmitEdges = 1u << 30, kSubjEmitIds = 2u << 30, kSubjChild = 3u << 30;  // task kinds (tag bits 30-31)
constexpr uint32_t kSubjTagMasked = 1u << 22;  // task tag (bits 22-29 are free): the row is the one that holds the relationship left out (RevokePolicy)
namespace {
// ORs bit `id` into the result row; lanes holding the same 32-bit word (ascending ids of one row) fold their bits first and one lane issues the atomic.
// Call in wave-uniform control flow.
__device__ __forceinline__ void subj_mark(uint32_t *row, bool lds, uint32_t id, bool valid, uint32_t nbits, uint32_t lane) {
    valid = valid && id < nbits;
    const uint32_t w = valid ? id >> 5 : 0xFFFFFFFFu;
    uint32_t b = valid ? 1u << (id & 31u) : 0u;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t ow = (uint32_t)__shfl_down((int)w, d), ob = (uint32_t)__shfl_down((int)b, d);
        if (lane + (uint32_t)d < 64u && ow == w) b |= ob;
    }
    const uint32_t pw = (uint32_t)__shfl_up((int)w, 1);
    if (valid && (lane == 0u || pw != w)) {
        if (lds) atomicOr(row + w, b);
        else __hip_atomic_fetch_or(row + w, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

struct SubjTables {  // what the decode reads: global memory, or a block's staged copy of the first three (subj_stage_programs)
    const SlotProg *progs;
    const FwdOp *ops;
    const SubjOp *sops;
    const uint2 *__restrict__ meta2, *__restrict__ smeta2;  // {first, end} of the sorted rows / of the subject rows
};
__device__ __forceinline__ SubjTables subj_tables(const DevSubjects &g) {
    return SubjTables{g.progs, g.ops, g.sops, reinterpret_cast<const uint2 *>(g.meta), reinterpret_cast<const uint2 *>(g.smeta)};
}
// copies [programs | ops | side table] into dynamic LDS and points T at the copies; returns the first word behind them (no barrier: the caller's follows)
__device__ __forceinline__ uint32_t *subj_stage_programs(const DevSubjects &g, uint4 *s_dyn, SubjTables &T, uint32_t tid) {
    SlotProg *lp = reinterpret_cast<SlotProg *>(s_dyn);
    FwdOp *lo = reinterpret_cast<FwdOp *>(lp + g.nslots);
    SubjOp *ls = reinterpret_cast<SubjOp *>(lo + g.nops);
    for (uint32_t i = tid; i < g.nslots; i += kSubjThreads) lp[i] = g.progs[i];
    for (uint32_t i = tid; i < g.nops; i += kSubjThreads) {
        lo[i] = g.ops[i];
        ls[i] = g.sops[i];
    }
    T.progs = lp;
    T.ops = lo;
    T.sops = ls;
    return reinterpret_cast<uint32_t *>(ls + g.nops);
}

struct SubjStep {  // what one (state, op) pair asks of the walk
    uint32_t start = 0, deg = 0, tag = 0;  // a row to walk: [start, start + deg) of g.sids (kSubjEmitIds) or g.edges; tag = kind | child level << 16 | child slot
    uint32_t one_slot = 0, one_lvl = 0;
    uint32_t flags = 0;  // (bits of one word, not four booleans: a divergent boolean that outlives its branch is a 64-bit lane mask)
    static constexpr uint32_t kOneChild = 1u;  // the state's own object is a child state (OP_PUSH_SAME)
    static constexpr uint32_t kOneEmit = 2u;   // the state's own id is a subject (OP_REFLEX); TEST: this op finds the item's subject
    static constexpr uint32_t kWild = 4u;      // a `T:*` row was reached (never with TEST: the wildcard's row is tested like any other)
    static constexpr uint32_t kTooLong = 8u;   // a row beyond kSubjMaxRow that the walk would have to enumerate
    __device__ __forceinline__ bool one_child() const { return (flags & kOneChild) != 0u; }
    __device__ __forceinline__ bool one_emit() const { return (flags & kOneEmit) != 0u; }
    __device__ __forceinline__ bool wild() const { return (flags & kWild) != 0u; }
    __device__ __forceinline__ bool too_long() const { return (flags & kTooLong) != 0u; }
};
// what a probe does (subj_decode's mode): LookupSubjects hands the probed row back to be emitted, Explain tests it for the item's one subject, Explain
// denial ignores it (the closure of a resource's states is the same for every subject)
struct SubjEmit {
    static constexpr bool kTest = false, kReach = false;
    __device__ __forceinline__ bool is(uint32_t) const { return true; }
    __device__ __forceinline__ bool hashed_has(const FwdOp &, uint32_t, uint32_t) const { return false; }
    __device__ __forceinline__ bool sorted_has(const uint2 &, uint32_t, uint32_t) const { return false; }
};
struct SubjReach {
    static constexpr bool kTest = false, kReach = true;
    __device__ __forceinline__ bool is(uint32_t) const { return false; }
    __device__ __forceinline__ bool hashed_has(const FwdOp &, uint32_t, uint32_t) const { return false; }
    __device__ __forceinline__ bool sorted_has(const uint2 &, uint32_t, uint32_t) const { return false; }
};
struct SubjTest {
    static constexpr bool kTest = true, kReach = false;
    const DevGraph *dg;  // what subject_row_contains reads: the forward row descriptors and the hashed buckets
    uint32_t sid;
    __device__ __forceinline__ bool is(uint32_t id) const { return id == sid; }
    __device__ __forceinline__ bool hashed_has(const FwdOp &op, uint32_t, uint32_t id) const { return subject_row_contains(*dg, op, id, sid); }
    __device__ __forceinline__ bool sorted_has(const uint2 &md, uint32_t, uint32_t) const { return row_contains(dg->edges, md.x, md.y, sid); }
};
// Explain for revocation: SubjTest with ONE stored relationship left out (engine_revoke.cpp).  The relationship is {class, resource id, subject id}; `cls`
// numbers the class of relationships every op reads (one word per FwdOp; a `T:*` class has a number of its own, so an OP_WILD op's class says that the
// row tested is the wildcard's).  A terminal hit of an op of the mask's class at the mask's resource does not count when the subject it tests is the mask's:
// the item's own, or -- the class being a wildcard's -- `T:*`, whoever asks.
struct SubjMask {
    uint32_t cls, rid, sid, wild;
};
struct SubjTestMasked {
    static constexpr bool kTest = true, kReach = false;
    SubjTest t;
    const uint32_t *__restrict__ cls;
    SubjMask m;
    __device__ __forceinline__ bool is(uint32_t id) const { return t.is(id); }
    __device__ __forceinline__ bool masked(uint32_t opi, uint32_t id) const { return gld(cls, opi) == m.cls && id == m.rid && (m.wild != 0u || t.sid == m.sid); }
    __device__ __forceinline__ bool hashed_has(const FwdOp &op, uint32_t opi, uint32_t id) const { return t.hashed_has(op, opi, id) && !masked(opi, id); }
    __device__ __forceinline__ bool sorted_has(const uint2 &md, uint32_t opi, uint32_t id) const { return t.sorted_has(md, opi, id) && !masked(opi, id); }
};
// Op j of the `nops` ops of program p that count for the state (p's slot, id) at `level`, looking for subjects of `key` (nops: n_total when the subject
// carries a relation -- REFLEX ops count -- else n_main; 0 for a lane without a state).  Side effects are the caller's: it turns `wild` and `too_long` into
// its own flag and stop code.  SubjTest: a probed row is tested, which also guards the id, and only ENUMERATED rows can be too long; SubjEmit: the probed
// row is handed back as a task, guarded by the side table's row count.  SubjReach: only OP_PUSH_SAME and OP_ENUM do anything (`key` is not read).
template <typename Mode>
__device__ __forceinline__ SubjStep subj_decode(const SubjTables &T, const SlotProg &p, uint32_t nops, uint32_t key, uint32_t id, uint32_t level, uint32_t j,
                                                const Mode &mode) {
    constexpr bool TEST = Mode::kTest, REACH = Mode::kReach;
    SubjStep d;
    if (j >= nops || (T.sops[p.first + j].flags & kSubjSkip)) return d;
    const FwdOp op = T.ops[p.first + j];
    const uint32_t L = level + op.dlevel;
    if (L > kMaxLevels) return d;
    if (op.flags & OP_REFLEX) {
        if (!REACH && op.key == key && mode.is(id)) d.flags = SubjStep::kOneEmit;
    } else if (op.flags & OP_PUSH_SAME) {
        if (L + 1u <= kMaxLevels) {
            d.flags = SubjStep::kOneChild;
            d.one_slot = op.key;
            d.one_lvl = L + 1u;
        }
    } else if (op.flags & OP_PROBE_HASH) {
        if (REACH || op.key != key) return d;
        if (TEST) {
            if (mode.hashed_has(op, p.first + j, id)) d.flags = SubjStep::kOneEmit;
            return d;
        }
        const SubjOp so = T.sops[p.first + j];
        if (id < so.nrows) {
            const uint2 rd = T.smeta2[so.base + id];
            if (rd.y > rd.x) {
                if (op.flags & OP_WILD) d.flags = SubjStep::kWild;
                else if (rd.y - rd.x > kSubjMaxRow) d.flags = SubjStep::kTooLong;
                else {
                    d.start = rd.x;
                    d.deg = rd.y - rd.x;
                    d.tag = kSubjEmitIds;
                }
            }
        }
    } else if (id < op.nrows) {
        const uint2 md = T.meta2[op.base + id * op.K + op.k];
        if (md.y > md.x) {
            const bool probe = !REACH && (op.flags & OP_PROBE) && op.key == key;
            const bool enm = (op.flags & OP_ENUM) && L + 1u <= kMaxLevels;
            if (TEST && probe && mode.sorted_has(md, p.first + j, id)) d.flags = SubjStep::kOneEmit;
            if (md.y - md.x > kSubjMaxRow) {
                if (enm || (!TEST && probe)) d.flags |= SubjStep::kTooLong;
            } else if (enm) {
                d.start = md.x;
                d.deg = md.y - md.x;
                d.tag = kSubjChild | ((L + 1u) << 16) | op.key;
            } else if (!TEST && probe) {
                d.start = md.x;
                d.deg = md.y - md.x;
                d.tag = kSubjEmitEdges;
            }
        }
    }
    return d;
}

// first visit of state (slot, id) of the lookup whose visited bits start at `visited`?  SCOPE: workgroup where the region is one block's own (the one-block
// walks), agent where the blocks of a launch share it (k_subj_expand: they sit on different XCDs, whose L2s are not coherent for anything less)
template <int SCOPE>
__device__ __forceinline__ bool subj_first_visit(const DevSubjects &g, uint32_t *__restrict__ visited, uint32_t slot, uint32_t id) {
    const uint32_t vb = g.slot_vbase[slot];
    if (vb == kSubjNoBits) return true;  // (nothing produces this slot's states: a lookup's own root)
    if (id >= g.slot_vn[slot]) return false;
    const uint32_t m = 1u << (id & 31u);
    return !(__hip_atomic_fetch_or(visited + vb + (id >> 5), m, __ATOMIC_RELAXED, SCOPE) & m);
}

struct SubjTaskLds {
    uint32_t start[kSubjThreads];
    uint32_t prefix[kSubjThreads + 1];
    uint32_t tag[kSubjThreads];  // kind | child level << 16 | child slot
};
struct ExplainTaskLds : SubjTaskLds {
    uint32_t parent[kSubjThreads];  // log index of the state the row belongs to
    uint32_t opi[kSubjThreads];     // index of the enumerating op
};
template <typename Tasks>
struct SubjWalkLds {  // the walk's static LDS, declared alignas(16).  The kernel's thread 0 sets end = 1 (the root is log[0]) and stop = 0 before the walk.
    uint32_t wave_tot[kSubjThreads / 64];  // (first: block_excl_scan reads them back as four 16-byte loads)
    uint32_t end, stop;
    Tasks t;
};

// The level loop of one block.  log[0] is the root, written by the kernel (which also decides whether the root's visit is marked there or left to stage A).
// Per level: read the log's end behind the previous round's barrier; stage A; rounds of kSubjThreads (state, op) pairs -- decode, the state's own emit and
// child, a block-wide scan of the degrees, then the lanes walk the concatenated rows (consecutive lanes, consecutive ids of one row); each round closes with
// one __syncthreads_or of the stop word.  Stops: 1 = the log is full (log_append), 2 = a row too long; the word is last-writer-wins within a round.
// Returns true when the policy's end-of-level test ended the walk, false when the log ran dry, the depth limit was reached or the walk stopped.
// The policy P supplies (its hooks run in wave-uniform control flow and contain no barrier):
//   Entry, entry(id, y, par, opi)   the log entry type; a child's entry from its producer (log index `par` of the parent state, op index `opi`)
//   Tasks, keep_producer, producer  the task list, and what a row's task remembers of its producer (log index, op index, object id) for its children
//   left_out(tag, v)                child v of the row whose task carries `tag` is not a child at all (Explain for revocation: the relationship left out,
//                                   which keep_producer marked in the tag); false for every other policy, where it compiles to nothing
//   probe                           the decode's mode (SubjEmit / SubjTest / SubjTestMasked / SubjReach)
//   state(step, id, me, opi, lane)  the one-lane results of a pair: `wild`, and `one_emit` -- the state's own id is a subject / the op finds the subject
//   element(v, emit, lane)          one id of an emitted row
//   level_done(stop)                tested behind the last round of a level, before the stop
template <typename P>
__device__ __forceinline__ bool subj_block_walk(P &pol, const DevSubjects &g, const SubjTables &T, uint32_t key, typename P::Entry *log, uint32_t cap,
                                                uint32_t *__restrict__ visited, SubjWalkLds<typename P::Tasks> &w, uint32_t tid, uint32_t lane, uint32_t wib) {
    using Entry = typename P::Entry;
    const bool rel_key = key < g.nslots;  // the subject carries a relation: REFLEX ops count
    const uint32_t W = rel_key ? g.max_ops_rel : g.max_ops;
    constexpr bool only_children = decltype(pol.probe)::kTest || decltype(pol.probe)::kReach;
    // child (slot, id) at level lvl, produced while level `cur` is expanded
    auto child = [&](uint32_t id, uint32_t slot, uint32_t lvl, uint32_t cur, bool valid, uint32_t par, uint32_t opi) {
        bool push = false;
        uint32_t y = slot | (lvl << 16);
        if (valid) {
            if (lvl == cur + 1u) {
                push = subj_first_visit<__HIP_MEMORY_SCOPE_WORKGROUP>(g, visited, slot, id);
                y |= kSubjMarked;
            } else {
                push = true;
            }
        }
        log_append(log, cap, &w.end, &w.stop, lane, push, pol.entry(id, y, par, opi));
    };
    uint32_t lo = 0, level = 1;
    int stop = 0;
    for (; level <= kMaxLevels; level++) {
        const uint32_t hi = w.end;  // (behind the previous round's closing barrier)
        __syncthreads();            // (every wave has read it before the first append of this level moves it)
        if (hi == lo || hi > cap) break;
        // ---- stage A: entries of later levels move behind this one (as they are, producer included); unmarked entries of this level decide their visit now
        for (uint32_t b0 = lo; b0 < hi; b0 += kSubjThreads) {
            const uint32_t i = b0 + tid;
            bool later = false;
            Entry en = pol.entry(0u, 0u, 0u, 0u);
            if (i < hi) {
                en = log[i];
                const uint32_t lv = (en.y >> 16) & 63u;
                if (lv > level) {
                    later = true;
                    log[i].y = en.y | kSubjDead;
                } else if (!(en.y & kSubjMarked) && !subj_first_visit<__HIP_MEMORY_SCOPE_WORKGROUP>(g, visited, en.y & 0xFFFFu, en.x)) {
                    log[i].y = en.y | kSubjDead;
                }
            }
            en.y &= ~(kSubjMarked | kSubjDead);
            log_append(log, cap, &w.end, &w.stop, lane, later, en);
        }
        __syncthreads();
        // ---- stage B: (state, op) pairs, one per thread and round
        const uint32_t npairs = (hi - lo) * W;
        for (uint32_t pb = 0; pb < npairs; pb += kSubjThreads) {
            const uint32_t q = pb + tid;
            SubjStep d;
            uint32_t id = 0, me = 0, opi = 0;
            if (q < npairs) {
                const uint32_t e = q / W, j = q - e * W;
                me = lo + e;
                const Entry en = log[me];
                id = en.x;  // (read with y whatever the entry's state: one load of the whole entry; a dead entry's id is never used)
                if (!(en.y & kSubjDead)) {
                    const SlotProg p = T.progs[en.y & 0xFFFFu];
                    opi = p.first + j;
                    d = subj_decode(T, p, rel_key ? p.n_total : p.n_main, key, id, level, j, pol.probe);
                }
            }
            if (d.too_long()) w.stop = 2u;
            pol.state(d, id, me, opi, lane);
            child(id, d.one_slot, d.one_lvl, level, d.one_child(), me, opi);
            uint32_t before, total;
            block_excl_scan<kSubjThreads>(d.deg, lane, wib, w.wave_tot, before, total);
            if (total) {  // (block-uniform)
                w.t.prefix[tid] = before;
                w.t.start[tid] = d.start;
                w.t.tag[tid] = d.tag;
                pol.keep_producer(w.t, tid, me, opi, id);
                __syncthreads();
                for (uint32_t wb = 0; wb < total; wb += kSubjThreads) {
                    const uint32_t x = wb + tid;
                    const bool valid = x < total;
                    const uint32_t xv = valid ? x : total - 1u;  // (inactive lanes shadow the last id: every load stays in range)
                    const uint32_t jt = task_owner<kSubjThreads>(w.t.prefix, xv);
                    const uint32_t tg = w.t.tag[jt], kind = only_children ? kSubjChild : tg & (3u << 30);  // (TEST, REACH: rows are only ever enumerated)
                    const uint32_t pos = w.t.start[jt] + (xv - w.t.prefix[jt]);
                    const uint32_t v = kind == kSubjEmitIds ? gld(g.sids, pos) : (gld(g.edges, pos) & kIdMask);
                    pol.element(v, valid && kind != kSubjChild, lane);
                    const uint2 from = pol.producer(w.t, jt);
                    child(v, tg & 0xFFFFu, (tg >> 16) & 63u, level, valid && kind == kSubjChild && !pol.left_out(tg, v), from.x, from.y);
                }
            }
            // (also the barrier behind the task list: every lane is done with it before the next round overwrites it)
            stop = __syncthreads_or(w.stop != 0u);
            if (stop) break;
        }
        if (pol.level_done(w.stop)) return true;  // (behind a barrier either way: block-uniform)
        if (stop) break;
        lo = hi;
    }
    return false;
}

struct SubjectsPolicy {  // LookupSubjects: 8-byte entries {id, slot | level << 16 | marks}; subjects are marked in the lookup's row
    using Entry = uint2;
    using Tasks = SubjTaskLds;
    uint32_t *row;
    bool row_lds;
    uint32_t nbits;
    uint32_t *s_wild;
    SubjEmit probe;
    __device__ __forceinline__ Entry entry(uint32_t id, uint32_t y, uint32_t, uint32_t) const { return make_uint2(id, y); }
    __device__ __forceinline__ void keep_producer(Tasks &, uint32_t, uint32_t, uint32_t, uint32_t) const {}
    __device__ __forceinline__ bool left_out(uint32_t, uint32_t) const { return false; }
    __device__ __forceinline__ uint2 producer(const Tasks &, uint32_t) const { return make_uint2(0u, 0u); }
    __device__ __forceinline__ void state(const SubjStep &d, uint32_t id, uint32_t, uint32_t, uint32_t lane) const {
        if (d.wild()) *s_wild = 1u;
        subj_mark(row, row_lds, id, d.one_emit(), nbits, lane);
    }
    __device__ __forceinline__ void element(uint32_t v, bool emit, uint32_t lane) const { subj_mark(row, row_lds, v, emit, nbits, lane); }
    __device__ __forceinline__ bool level_done(uint32_t) const { return false; }
};
struct ExplainPolicy {  // Explain: 16-byte entries that also carry {log index of the parent, index of the op that produced the state}; the first hit ends the walk
    using Entry = uint4;
    using Tasks = ExplainTaskLds;
    SubjTest probe;
    unsigned long long *s_hit;  // min over the hits of (log index << 32 | op index)
    __device__ __forceinline__ Entry entry(uint32_t id, uint32_t y, uint32_t par, uint32_t opi) const { return make_uint4(id, y, par, opi); }
    __device__ __forceinline__ bool left_out(uint32_t, uint32_t) const { return false; }
    __device__ __forceinline__ void keep_producer(Tasks &t, uint32_t tid, uint32_t me, uint32_t opi, uint32_t) const {
        t.parent[tid] = me;
        t.opi[tid] = opi;
    }
    __device__ __forceinline__ uint2 producer(const Tasks &t, uint32_t jt) const { return make_uint2(t.parent[jt], t.opi[jt]); }
    __device__ __forceinline__ void state(const SubjStep &d, uint32_t, uint32_t me, uint32_t opi, uint32_t) const {
        if (d.one_emit()) atomicMin(s_hit, ((unsigned long long)me << 32) | opi);
    }
    __device__ __forceinline__ void element(uint32_t, bool, uint32_t) const {}
    // A log that overflowed on children of the level that found the subject does not matter: the hit state and its ancestors were appended before this level
    // began, and nothing below them is needed.  An enumerated row beyond the limit (2) still fails.  (The stop word is last-writer-wins: an append's 1 may
    // overwrite a 2 of the same round.  That only decides whether a witness already found is returned; it is valid either way.)
    __device__ __forceinline__ bool level_done(uint32_t stop) const { return *s_hit != ~0ull && stop != 2u; }
};
struct RevokePolicy {  // Explain for revocation: Explain's tests with one relationship left out; 8-byte entries (no path is traced back); the first hit ends the walk
    using Entry = uint2;
    using Tasks = SubjTaskLds;
    SubjTestMasked probe;
    uint32_t *s_found;
    __device__ __forceinline__ Entry entry(uint32_t id, uint32_t y, uint32_t, uint32_t) const { return make_uint2(id, y); }
    // the row of (an op of the mask's class, the mask's resource) is the one row that can hold the relationship: its task says so in its tag
    __device__ __forceinline__ void keep_producer(Tasks &t, uint32_t tid, uint32_t, uint32_t opi, uint32_t id) const {
        if (t.tag[tid] != 0u && id == probe.m.rid && gld(probe.cls, opi) == probe.m.cls) t.tag[tid] |= kSubjTagMasked;
    }
    __device__ __forceinline__ bool left_out(uint32_t tag, uint32_t v) const { return (tag & kSubjTagMasked) != 0u && v == probe.m.sid; }
    __device__ __forceinline__ uint2 producer(const Tasks &, uint32_t) const { return make_uint2(0u, 0u); }
    __device__ __forceinline__ void state(const SubjStep &d, uint32_t, uint32_t, uint32_t, uint32_t) const {
        if (d.one_emit()) *s_found = 1u;
    }
    __device__ __forceinline__ void element(uint32_t, bool, uint32_t) const {}
    // as ExplainPolicy's: a hit stands whatever the log did at the level that produced it; an enumerated row beyond the limit still fails
    __device__ __forceinline__ bool level_done(uint32_t stop) const { return *s_found != 0u && stop != 2u; }
};
struct ReachPolicy {  // Explain denial: 8-byte entries as LookupSubjects'; nothing is emitted or tested and no level ends the walk -- the log is the result
    using Entry = uint2;
    using Tasks = SubjTaskLds;
    SubjReach probe;
    __device__ __forceinline__ Entry entry(uint32_t id, uint32_t y, uint32_t, uint32_t) const { return make_uint2(id, y); }
    __device__ __forceinline__ void keep_producer(Tasks &, uint32_t, uint32_t, uint32_t, uint32_t) const {}
    __device__ __forceinline__ bool left_out(uint32_t, uint32_t) const { return false; }
    __device__ __forceinline__ uint2 producer(const Tasks &, uint32_t) const { return make_uint2(0u, 0u); }
    __device__ __forceinline__ void state(const SubjStep &, uint32_t, uint32_t, uint32_t, uint32_t) const {}
    __device__ __forceinline__ void element(uint32_t, bool, uint32_t) const {}
    __device__ __forceinline__ bool level_done(uint32_t) const { return false; }
};
}  // namespace

// LookupSubjects, one block per lookup: setup, subj_block_walk, then the row and the wildcard flag go out.  The root is appended UNMARKED: stage A of the first
// level decides its visit, so a resource id beyond its slot's visited bits is not walked.
__global__ __launch_bounds__(kSubjThreads) void k_subj_local(DevSubjects g, const uint32_t *__restrict__ rids, uint32_t target_slot, uint32_t key, uint2 *logs,
                                                             uint32_t cap, uint32_t *visited_all, uint32_t *rows, uint32_t row_words, uint32_t lds_words, uint32_t prog_lds,
                                                             uint32_t *flags_out, uint32_t *status) {
    __shared__ alignas(16) SubjWalkLds<SubjTaskLds> w;
    __shared__ uint32_t s_wild;
    // dynamic LDS: [programs | ops | side table] when prog_lds, then the result row when lds_words
    extern __shared__ uint4 s_dyn[];
    const uint32_t tid = threadIdx.x, lane = lane_id(), wib = tid >> 6;
    const uint32_t req = blockIdx.x;
    SubjTables T = subj_tables(g);
    uint32_t *const dyn_words = prog_lds ? subj_stage_programs(g, s_dyn, T, tid) : reinterpret_cast<uint32_t *>(s_dyn);
    const bool row_lds = lds_words != 0u;
    uint32_t *const row = row_lds ? dyn_words : rows + (size_t)req * row_words;
    uint2 *const log = logs + (size_t)req * cap;
    for (uint32_t i = tid; i < lds_words; i += kSubjThreads) row[i] = 0u;
    if (tid == 0) {
        w.end = 1;
        w.stop = 0;
        s_wild = 0;
        log[0] = make_uint2(rids[req], target_slot | (1u << 16));
    }
    __syncthreads();
    SubjectsPolicy pol{row, row_lds, row_words * 32u, &s_wild, SubjEmit{}};
    subj_block_walk(pol, g, T, key, log, cap, visited_all + (size_t)req * g.visited_words, w, tid, lane, wib);
    __syncthreads();
    if (tid == 0) {
        if (w.stop) *status = w.stop;
        flags_out[req] = s_wild;
    }
    if (row_lds) {
        uint32_t *orow = rows + (size_t)req * row_words;
        for (uint32_t i = tid; i < row_words; i += kSubjThreads) orow[i] = i < lds_words ? row[i] : 0u;
    }
}

// bytes of [programs | ops | side table]; staged in the walking block's LDS when they fit kSubjLdsProgBytes
static size_t subj_prog_bytes(const DevSubjects &g) { return (size_t)g.nslots * sizeof(SlotProg) + (size_t)g.nops * (sizeof(FwdOp) + sizeof(SubjOp)); }

void launch_subj_local(hipStream_t s, const DevSubjects &g, const uint32_t *rids, uint32_t n, uint32_t target_slot, uint32_t key, void *logs, uint32_t cap,
                       uint32_t *visited, uint32_t *rows, uint32_t row_words, uint32_t *flags_out, uint32_t *status) {
    if (!n) return;
    static const bool big_lds =
        hipFuncSetAttribute(reinterpret_cast<const void *>(k_subj_local), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kRevLdsRowBytes + kSubjLdsProgBytes)) == hipSuccess;
    const size_t prog_bytes = subj_prog_bytes(g);
    const uint32_t prog_lds = prog_bytes <= kSubjLdsProgBytes ? 1u : 0u;
    const uint32_t lds_words = (size_t)row_words * 4u <= (big_lds ? kRevLdsRowBytes : 16384u) ? row_words : 0u;
    const size_t dyn = (prog_lds ? prog_bytes : 0u) + (size_t)lds_words * 4u;
    hipLaunchKernelGGL(k_subj_local, dim3(n), dim3(kSubjThreads), dyn, s, g, rids, target_slot, key, (uint2 *)logs, cap, visited, rows, row_words, lds_words, prog_lds,
                       flags_out, status);
}

// ---- Explain: k_explain_local (engine_explain.cpp).  One block walks ONE item -- from the item's resource down the forward programs, subj_block_walk with
// ExplainPolicy -- and where LookupSubjects emits the ids of a row, this walk TESTS the row for the item's one subject, with the device functions k_check_local's
// interpreter uses (subject_row_contains, row_contains): a hit here is a hit of Check's.  Log entries are 16 bytes and carry how the state was reached:
// {id, slot | level << 16 | marks, log index of the parent, index of the op that produced it}.  The log discipline and the depth arithmetic are the shared
// walk's, so a state counts at the least level it can be reached at and a witness exists exactly where Check answers HAS.  A hit does an LDS atomicMin of
// (log index << 32 | op index); the walk ends behind the first level that produced one and one lane follows the parent indices back to entry 0, writing
// {op, parent id, child id, flags} records in path order.
__global__ __launch_bounds__(kSubjThreads) void k_explain_local(DevSubjects g, const uint32_t *__restrict__ buckets, const uint4 *__restrict__ items, uint4 *logs,
                                                                uint32_t cap, uint32_t *visited_all, uint32_t prog_lds, uint4 *__restrict__ traces,
                                                                uint32_t *__restrict__ counts, uint32_t *status) {
    __shared__ alignas(16) SubjWalkLds<ExplainTaskLds> w;
    __shared__ unsigned long long s_hit;
    extern __shared__ uint4 s_dyn[];  // [programs | ops | side table] when prog_lds
    const uint32_t tid = threadIdx.x, lane = lane_id(), wib = tid >> 6;
    const uint32_t req = blockIdx.x;
    SubjTables T = subj_tables(g);
    if (prog_lds) (void)subj_stage_programs(g, s_dyn, T, tid);
    const uint4 item = items[req];  // {resource id, target slot, subject key, subject id}
    const uint32_t sid = item.w;
    uint32_t *__restrict__ visited = visited_all + (size_t)req * g.visited_words;
    uint4 *const log = logs + (size_t)req * cap;
    if (tid == 0) {
        w.end = 1;
        w.stop = 0;
        s_hit = ~0ull;
        log[0] = make_uint4(item.x, item.y | (1u << 16) | kSubjMarked, 0u, 0u);  // (the root is walked whatever its id: an object no relationship names can still be its own subject)
    }
    __syncthreads();
    DevGraph dg{};  // (what subject_row_contains reads: the forward row descriptors and the hashed buckets)
    dg.meta = g.meta;
    dg.edges = g.edges;
    dg.buckets = buckets;
    if (tid == 0) (void)subj_first_visit<__HIP_MEMORY_SCOPE_WORKGROUP>(g, visited, item.y, item.x);  // (the root's MARKED entry: ordered before every other visit by the first level's barriers)
    ExplainPolicy pol{SubjTest{&dg, sid}, &s_hit};
    const bool found = subj_block_walk(pol, g, T, item.z, log, cap, visited, w, tid, lane, wib);
    __syncthreads();
    if (tid != 0) return;
    // ---- back-trace (one lane): at most kMaxLevels states lie on a path (their levels ascend), every index is checked before it is followed
    if (w.stop && !found) {
        *status = w.stop;
        counts[req] = 1u << 16;
        return;
    }
    if (!found) {
        counts[req] = 1u << 16;  // not found
        return;
    }
    const uint32_t end = min(w.end, cap);
    const uint32_t h = (uint32_t)(s_hit >> 32), ho = (uint32_t)s_hit;
    uint32_t depth = 0, i = h;
    bool bad = h >= end || ho >= g.nops;
    for (uint32_t k = 0; !bad && k < kMaxLevels && i != 0u; k++) {
        const uint32_t par = log[i].z;
        if (par >= end || par >= i) bad = true;  // (a parent was appended before its child)
        i = par;
        depth++;
    }
    if (bad || i != 0u) {
        counts[req] = 2u << 16;  // the log does not lead back to the item's resource
        return;
    }
    uint4 *const rec = traces + (size_t)req * (kMaxLevels + 1u);
    uint32_t n = depth;
    const FwdOp fo = T.ops[ho];
    if (!(fo.flags & OP_REFLEX)) {
        const bool wild = (fo.flags & OP_WILD) != 0u;
        rec[n++] = make_uint4(ho, log[h].x, wild ? fo.K : sid, wild ? 1u : 0u);
    }
    i = h;
    for (uint32_t k = depth; k > 0u; k--) {
        const uint4 en = log[i];
        const uint32_t par = en.z < end ? en.z : 0u;
        rec[k - 1u] = make_uint4(en.w, log[par].x, en.x, 0u);
        i = par;
    }
    counts[req] = n;
}

void launch_explain_local(hipStream_t s, const DevSubjects &g, const uint32_t *buckets, const uint4 *items, uint32_t n, void *logs, uint32_t cap, uint32_t *visited,
                          uint4 *traces, uint32_t *counts, uint32_t *status) {
    if (!n) return;
    const size_t prog_bytes = subj_prog_bytes(g);
    const uint32_t prog_lds = prog_bytes <= kSubjLdsProgBytes ? 1u : 0u;
    hipLaunchKernelGGL(k_explain_local, dim3(n), dim3(kSubjThreads), prog_lds ? prog_bytes : 0u, s, g, buckets, items, (uint4 *)logs, cap, visited, prog_lds, traces,
                       counts, status);
}

// ---- Explain for revocation: k_revoke_local (engine_revoke.cpp).  One block walks ONE (item, relationship left out): k_explain_local's walk from the item's
// resource, with RevokePolicy -- the terminal tests and the enumerated rows read every stored relationship but the mask's.  Nothing is traced back: the block
// answers one word, found (the grant survives the delete), not found (the delete revokes it: the walk ran the closure dry within the 50 dispatch levels) or
// stopped (the log overflowed before a hit, or a row beyond the limit: the host redoes the chunk or fails).  The log discipline and the depth arithmetic
// are the shared walk's, so the answer is the one a Check gives once the relationship is gone.
__global__ __launch_bounds__(kSubjThreads) void k_revoke_local(DevSubjects g, const uint32_t *__restrict__ buckets, const uint32_t *__restrict__ op_class,
                                                               const uint4 *__restrict__ recs, uint2 *logs, uint32_t cap, uint32_t *visited_all, uint32_t prog_lds,
                                                               uint32_t *__restrict__ found_out, uint32_t *status) {
    __shared__ alignas(16) SubjWalkLds<SubjTaskLds> w;
    __shared__ uint32_t s_found;
    extern __shared__ uint4 s_dyn[];  // [programs | ops | side table] when prog_lds
    const uint32_t tid = threadIdx.x, lane = lane_id(), wib = tid >> 6;
    const uint32_t req = blockIdx.x;
    SubjTables T = subj_tables(g);
    if (prog_lds) (void)subj_stage_programs(g, s_dyn, T, tid);
    const uint4 item = recs[2u * req];       // {resource id, target slot, subject key, subject id}
    const uint4 mask = recs[2u * req + 1u];  // {class, resource id, subject id, 1: the class is a wildcard's}
    uint32_t *__restrict__ visited = visited_all + (size_t)req * g.visited_words;
    uint2 *const log = logs + (size_t)req * cap;
    if (tid == 0) {
        w.end = 1;
        w.stop = 0;
        s_found = 0;
        log[0] = make_uint2(item.x, item.y | (1u << 16) | kSubjMarked);  // (walked whatever its id, as Explain's root)
        (void)subj_first_visit<__HIP_MEMORY_SCOPE_WORKGROUP>(g, visited, item.y, item.x);
    }
    __syncthreads();
    DevGraph dg{};  // (what subject_row_contains reads: the forward row descriptors and the hashed buckets)
    dg.meta = g.meta;
    dg.edges = g.edges;
    dg.buckets = buckets;
    RevokePolicy pol{SubjTestMasked{SubjTest{&dg, item.w}, op_class, SubjMask{mask.x, mask.y, mask.z, mask.w}}, &s_found};
    const bool found = subj_block_walk(pol, g, T, item.z, log, cap, visited, w, tid, lane, wib);
    __syncthreads();
    if (tid != 0) return;
    if (found) {
        found_out[req] = kRevokeFound;
    } else if (w.stop) {
        *status = w.stop;
        found_out[req] = kRevokeStopped;
    } else {
        found_out[req] = kRevokeNotFound;
    }
}

void launch_revoke_local(hipStream_t s, const DevSubjects &g, const uint32_t *buckets, const uint32_t *op_class, const uint4 *recs, uint32_t n, void *logs,
                         uint32_t cap, uint32_t *visited, uint32_t *found_out, uint32_t *status) {
    if (!n) return;
    const size_t prog_bytes = subj_prog_bytes(g);
    const uint32_t prog_lds = prog_bytes <= kSubjLdsProgBytes ? 1u : 0u;
    hipLaunchKernelGGL(k_revoke_local, dim3(n), dim3(kSubjThreads), prog_lds ? prog_bytes : 0u, s, g, buckets, op_class, recs, (uint2 *)logs, cap, visited, prog_lds,
                       found_out, status);
}

// ---- Explain denial: k_reach_local (engine_denial.cpp).  One block walks ONE distinct (resource, permission) of the call with ReachPolicy: the forward closure
// of the resource's state over userset and arrow relationships, which is the set of states a Check of that permission on that resource looks at whoever the
// subject is.  When the walk is over, the log's entries without kSubjDead are the distinct states, each at its least level (a second visit and an entry that was
// moved behind its level are dead; every other entry decided its first visit).  The block counts them, reserves that many records of the call-wide output region
// with one agent-scope add (the blocks sit on different XCDs) and copies them there in tiles of kSubjThreads behind a block-wide scan of the keep flags.  A block
// whose records do not fit raises *out.overflow and copies nothing: the host redoes the pass with a larger region.
__global__ __launch_bounds__(kSubjThreads) void k_reach_local(DevSubjects g, const uint2 *__restrict__ roots, uint2 *logs, uint32_t cap, uint32_t *visited_all,
                                                              uint32_t prog_lds, DevReachOut out, uint32_t *status) {
    __shared__ alignas(16) SubjWalkLds<SubjTaskLds> w;
    __shared__ uint32_t s_base;
    extern __shared__ uint4 s_dyn[];  // [programs | ops | side table] when prog_lds
    const uint32_t tid = threadIdx.x, lane = lane_id(), wib = tid >> 6;
    const uint32_t req = blockIdx.x;
    SubjTables T = subj_tables(g);
    if (prog_lds) (void)subj_stage_programs(g, s_dyn, T, tid);
    const uint2 root = roots[req];  // {resource id, target slot}
    uint32_t *__restrict__ visited = visited_all + (size_t)req * g.visited_words;
    uint2 *const log = logs + (size_t)req * cap;
    if (tid == 0) {
        w.end = 1;
        w.stop = 0;
        log[0] = make_uint2(root.x, root.y | (1u << 16) | kSubjMarked);  // (walked whatever its id, as Explain's root: a resource nobody has written is still a state)
        (void)subj_first_visit<__HIP_MEMORY_SCOPE_WORKGROUP>(g, visited, root.y, root.x);
    }
    __syncthreads();
    ReachPolicy pol{};
    (void)subj_block_walk(pol, g, T, 0xFFFFFFFFu /* no subject key: REFLEX ops do not count */, log, cap, visited, w, tid, lane, wib);
    __syncthreads();
    if (w.stop) {  // (block-uniform: read behind the barrier, written by nobody from here on)
        if (tid == 0) {
            *status = w.stop;
            out.spans[req] = make_uint2(0u, 0u);
        }
        return;
    }
    const uint32_t end = min(w.end, cap);
    uint32_t mine = 0;
    for (uint32_t i = tid; i < end; i += kSubjThreads) mine += (log[i].y & kSubjDead) ? 0u : 1u;
    uint32_t before, total;
    block_excl_scan<kSubjThreads>(mine, lane, wib, w.wave_tot, before, total);
    if (tid == 0) {
        const unsigned long long at = __hip_atomic_fetch_add(out.total, (unsigned long long)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool fits = at + total <= (unsigned long long)out.cap;
        if (!fits) *out.overflow = 1u;
        s_base = fits ? (uint32_t)at : 0xFFFFFFFFu;
        out.spans[req] = fits ? make_uint2((uint32_t)at, total) : make_uint2(0u, 0u);
    }
    __syncthreads();  // (also between the scan above and the first tile's)
    const uint32_t base = s_base;
    if (base == 0xFFFFFFFFu) return;
    uint32_t done = 0;
    for (uint32_t t0 = 0; t0 < end; t0 += kSubjThreads) {
        const uint32_t i = t0 + tid;
        uint2 en = make_uint2(0u, 0u);
        bool keep = false;
        if (i < end) {
            en = log[i];
            keep = !(en.y & kSubjDead);
        }
        uint32_t bf, tt;
        block_excl_scan<kSubjThreads>(keep ? 1u : 0u, lane, wib, w.wave_tot, bf, tt);
        if (keep) out.recs[(size_t)base + done + bf] = make_uint2(en.x, en.y & 0x3FFFFFu);  // (done + bf < total: inside the block's reservation)
        done += tt;
        __syncthreads();  // (the wave totals are read before the next tile's scan stores its own)
    }
}

void launch_reach_local(hipStream_t s, const DevSubjects &g, const uint2 *roots, uint32_t n, void *logs, uint32_t cap, uint32_t *visited, const DevReachOut &out,
                        uint32_t *status) {
    if (!n) return;
    const size_t prog_bytes = subj_prog_bytes(g);
    const uint32_t prog_lds = prog_bytes <= kSubjLdsProgBytes ? 1u : 0u;
    hipLaunchKernelGGL(k_reach_local, dim3(n), dim3(kSubjThreads), prog_lds ? prog_bytes : 0u, s, g, roots, (uint2 *)logs, cap, visited, prog_lds, out, status);
}

// ---- LookupSubjects, level-synchronous: k_subj_expand (the sharded graph's native loop, engine_shard_subjects.cpp).  One launch = one dispatch level of ALL
// lookups of a chunk on all CUs, over the chunked frontier of k_expand / k_rev_expand.  Entry: x = object id, y = lookup index, z = slot | level << 16 |
// kSubjMarked, w = 0.  What an op does is subj_decode's, as in the one-block walk (subj_block_walk); what differs is WHEN a visit is decided.  There, unmarked
// entries of level L decide behind a block barrier that follows every append of level L - 1.  Here other blocks (and other shards) are still appending, so
// every decision for a level-L state is taken while iteration L - 1 runs: where an L - 1 state's direct child is appended, where an entry that becomes due
// next is carried over, and where an exchanged entry is imported.  Entries of later levels travel unmarked.  Every visited bit set during iteration L - 1
// therefore belongs to level L, and a state still counts at the least level that reaches it -- across blocks and across shards (the bits live on the shard
// that owns the slot's type, and only there).  Iteration L reads: marked entries of level L (expanded), unmarked entries of levels > L (carried).
namespace {
__device__ __forceinline__ bool subj_first_visit(const DevSubjLevel &s, uint32_t req, uint32_t slot, uint32_t id) {
    return subj_first_visit<__HIP_MEMORY_SCOPE_AGENT>(s.g, s.visited + (size_t)req * s.g.visited_words, slot, id);
}
// wave-cooperative append of the flagged lanes' entries to the frontier iteration `iter` produces (wave-uniform control flow)
__device__ __forceinline__ void subj_append(WaveOut &wo, uint32_t lane, bool push, uint32_t id, uint32_t req, uint32_t z) {
    const uint64_t b = __ballot(push);
    if (!b) return;
    const uint32_t base = reserve<false>(wo, (uint32_t)__popcll(b), lane);
    if (push && base != kNoSpace) wo.buf[base + lanes_below(b)] = make_uint4(id, req, z, 0u);
}
// child state (slot, id) of lookup `req` at level lvl, produced while level `iter` is expanded: to the owner of the slot's type when that is another shard
// (unmarked: the importer decides), else into the next frontier -- its visit decided here when it is due next
template <bool SHARDED>
__device__ __forceinline__ void subj_child(const DevSubjLevel &s, WaveOut &wo, const DevShard &sh, uint32_t iter, uint32_t lane, bool valid, uint32_t id, uint32_t req,
                                           uint32_t slot, uint32_t lvl) {
    uint32_t z = slot | (lvl << 16);
    bool local = valid;
    if (SHARDED) {
        const uint32_t owner = valid ? s.g.progs[slot].owner : sh.rank;
        local = valid && owner == sh.rank;
        export_entries(valid && owner != sh.rank, make_uint4(id, req, z, 0u), owner, lane, sh);
    }
    bool push = local;
    if (local && lvl == iter + 1u) {
        push = subj_first_visit(s, req, slot, id);
        z |= kSubjMarked;
    }
    subj_append(wo, lane, push, id, req, z);
}
}  // namespace

// lookup i of the chunk starts from resource rids[i] of `target_slot`, on the shard that owns the slot's type; also resets the status block (as k_rev_seed)
__global__ __launch_bounds__(256) void k_subj_seed(DevSubjLevel s, DevFrontier f, const uint32_t *__restrict__ rids, uint32_t n, uint32_t target_slot, DevShard sh) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t need = (n + kChunk - 1) / kChunk;
    const uint32_t readable = max(need, f.nwaves);
    if (i < kStatusWords) f.nchunks[i] = i == 0 ? (need > f.nwaves ? need - f.nwaves : 0u) : (i == kLevelSlots ? (n ? 1u : 0u) : 0u);
    if (i < readable) f.counts[0][i] = i < need ? min(kChunk, n - i * kChunk) : 0u;
    if (i >= n) return;
    const uint32_t id = rids[i];
    bool mine = sh.world <= 1u || s.g.progs[target_slot].owner == sh.rank;
    if (mine) mine = subj_first_visit(s, i, target_slot, id);  // (an id beyond the visited bits: no walk, as in the one-block walk)
    f.buf[0][i] = make_uint4(id, i, mine ? (target_slot | (1u << 16) | kSubjMarked) : kDeadMeta, 0u);
}

template <bool SHARDED>
__global__ __launch_bounds__(kBlock) void k_subj_expand(DevSubjLevel s, DevFrontier f, uint32_t iter, DevShard sh) {
    __shared__ WaveOutCold s_cold[kWavesPerBlock];
    __shared__ uint32_t s_slots[kWavesPerBlock][128];
    const uint32_t lane = lane_id();
    const uint32_t wib = uniform(threadIdx.x >> 6);
    const uint32_t wave = blockIdx.x * kWavesPerBlock + wib, nwaves = f.nwaves;
    const uint32_t pin = (iter + 1) & 1u;
    const uint32_t *__restrict__ in_counts = f.counts[pin];
    const bool live = !*f.overflow && f.any[iter - 1];
    const uint32_t C = live ? nwaves + min(f.nchunks[iter - 1], f.max_chunks - nwaves) : 0u;
    WaveOut wo = chunked_out(f, iter, wave, &s_cold[wib], lane);
    uint32_t *slots = s_slots[wib];
    ChunkWalk cw{f.buf[pin], lane, slots, 0ull};
    const DevSubjects &g = s.g;
    const bool rel_key = s.key < g.nslots;  // the subject carries a relation: REFLEX ops count
    const uint32_t nbits = s.row_words * 32u;
    const SubjTables T = subj_tables(g);
    // segment-major work order: k_expand's ChunkWalk (the fill counts of the wave's next 64 segment slots in one gather)
    const uint32_t nslot = C * kSegsPerChunk;
    for (uint32_t x0 = wave; x0 < nslot; x0 += 64 * nwaves) {
        const uint32_t xl = x0 + lane * nwaves;
        uint32_t lat = 0, lcnt = 0;
        if (xl < nslot) {
            const uint32_t ls = xl / C, lc = (xl % C + ls * 509u) % C;
            lcnt = in_counts[lc];
            lcnt = lcnt > ls * 64 ? lcnt - ls * 64 : 0u;  // entries of this slot's segment and beyond
            lat = lc * kChunk + ls * 64;
        }
        wave_lds_fence();  // (the previous round's readers are done)
        slots[lane] = lat;
        slots[64 + lane] = lcnt;
        cw.work = __ballot(lcnt != 0);
        wave_lds_fence();
        while (cw.work) {
            const int wl = __ffsll((unsigned long long)cw.work) - 1;
            cw.take();
            uint4 e;
            bool valid;
            cw.load(wl, e, valid);
            if (!valid) e.z = kDeadMeta;
            const uint32_t id = e.x, req = e.y, z = e.z;
            const bool act = valid && z != kDeadMeta;
            const uint32_t slot = z & 0xFFFFu, level = (z >> 16) & 63u;
            {  // entries of later levels move on; the ones due next decide their visit now
                const bool later = act && level > iter;
                bool push = later;
                uint32_t nz = z & ~kSubjMarked;
                if (later && level == iter + 1u) {
                    push = subj_first_visit(s, req, slot, id);
                    nz |= kSubjMarked;
                }
                subj_append(wo, lane, push, id, req, nz);
            }
            const bool expand = act && level == iter;  // (marked: its visit was decided during the iteration before)
            SlotProg p{};
            if (expand) p = g.progs[slot];
            const uint32_t nops = expand ? (rel_key ? p.n_total : p.n_main) : 0u;
            const uint32_t maxops = wave_max(nops);
            for (uint32_t j = 0; j < maxops; j++) {
                const SubjStep d = subj_decode(T, p, nops, s.key, id, level, j, SubjEmit{});
                if (d.wild()) s.flags[req] = 1;
                if (d.too_long()) *f.overflow = 2u;
                // the state itself is the subject (REFLEX): the lanes hold different lookups, so each ORs its own bit
                if (d.one_emit() && id < nbits)
                    __hip_atomic_fetch_or(s.rows + (size_t)req * s.row_words + (id >> 5), 1u << (id & 31u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                subj_child<SHARDED>(s, wo, sh, iter, lane, d.one_child(), id, req, d.one_slot, d.one_lvl);
                // rows: the wave walks one lane's row at a time, consecutive lanes on consecutive ids (coalesced; ascending ids fold in subj_mark)
                uint64_t todo = __ballot(d.deg != 0);
                while (todo) {
                    const int src = __ffsll((unsigned long long)todo) - 1;
                    todo &= todo - 1;
                    const uint32_t tstart = (uint32_t)__builtin_amdgcn_readlane((int)d.start, src), tdeg = (uint32_t)__builtin_amdgcn_readlane((int)d.deg, src);
                    const uint32_t ttag = (uint32_t)__builtin_amdgcn_readlane((int)d.tag, src), treq = (uint32_t)__builtin_amdgcn_readlane((int)req, src);
                    const uint32_t kind = ttag & (3u << 30);
                    uint32_t *row = s.rows + (size_t)treq * s.row_words;
                    for (uint32_t o = 0; o < tdeg; o += 64) {
                        const bool v = o + lane < tdeg;
                        const uint32_t pos = tstart + (v ? o + lane : 0u);
                        const uint32_t val = kind == kSubjEmitIds ? gld(g.sids, pos) : (gld(g.edges, pos) & kIdMask);
                        if (kind != kSubjChild) subj_mark(row, false, val, v, nbits, lane);
                        else subj_child<SHARDED>(s, wo, sh, iter, lane, v, val, treq, ttag & 0xFFFFu, (ttag >> 16) & 63u);
                    }
                }
            }
        }
    }
    if (lane == 0) {
        if (wo.cur != kNoSpace) wo.cold->counts[wo.cur] = wo.fill;
        if (wo.produced) f.any[iter] = 1u;
    }
}

// After the exchange (k_import_gathered's shape: blockIdx.y = source shard; the own row's first wave folds the headers into the level's control record).
// Keeps the gathered entries whose slot this shard owns and appends them to the frontier iteration `iter` produced; an entry that is due next decides its
// visit here -- on its owner, in the same iteration as every other decision for that level.
__global__ __launch_bounds__(256) void k_subj_import_gathered(DevSubjLevel s, DevFrontier f, uint32_t iter, const uint4 *__restrict__ hdrs, const uint4 *__restrict__ data,
                                                              uint32_t world, uint32_t rank, uint32_t cap, uint32_t have_data, uint32_t *ctrl) {
    const uint32_t lane = lane_id();
    const uint4 *__restrict__ in;
    uint32_t n;
    if (!gathered_input(hdrs, data, world, rank, cap, have_data, ctrl, lane, &in, &n)) return;
    const uint32_t wave = blockIdx.x * 4 + (threadIdx.x >> 6), nw = gridDim.x * 4;
    ImportOut io(f, iter);
    for (uint32_t x = wave; (uint64_t)x * 64 < n; x += nw) {
        const uint32_t i = x * 64 + lane;
        uint4 e = i < n ? in[i] : make_uint4(0, 0, kDeadMeta, 0);
        bool mine = i < n && e.z != kDeadMeta;
        const uint32_t slot = e.z & 0xFFFFu;
        if (mine) mine = slot < s.g.nslots && s.g.progs[slot].owner == rank;
        if (mine && ((e.z >> 16) & 63u) == iter + 1u) {
            mine = subj_first_visit(s, e.y, slot, e.x);
            e.z |= kSubjMarked;
        }
        if (!io.append(mine, e, lane)) break;
    }
    io.close(lane);
}

// result rows: ORs the `world` gathered partial rows ([world][m][row_words]) into out[m][out_stride]; the words behind row_words are zeroed.  (Several
// shards set different bits of one byte -- pod#creator on pod's shard, group#member on group's -- so a byte-wise max would not do.)
__global__ __launch_bounds__(256) void k_subj_fold(const uint32_t *__restrict__ gathered, uint32_t world, uint32_t m, uint32_t row_words, uint32_t *out,
                                                   uint32_t out_stride) {
    const size_t total = (size_t)m * out_stride, part = (size_t)m * row_words;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / out_stride;
        const uint32_t w = (uint32_t)(i - r * out_stride);
        uint32_t v = 0;
        if (w < row_words)
            for (uint32_t k = 0; k < world; k++) v |= gathered[k * part + r * row_words + w];
        out[i] = v;
    }
}

void launch_subj_seed(hipStream_t st, const DevSubjLevel &s, const DevFrontier &f, const uint32_t *rids, uint32_t n, uint32_t target_slot, const DevShard &sh) {
    const uint32_t threads = std::max(std::max(n, f.nwaves), kStatusWords);
    hipLaunchKernelGGL(k_subj_seed, dim3((threads + 255) / 256), dim3(256), 0, st, s, f, rids, n, target_slot, sh);
}
void launch_subj_expand(hipStream_t st, const DevSubjLevel &s, const DevFrontier &f, uint32_t iter, const DevShard &sh) {
    const dim3 grid(f.nwaves / kWavesPerBlock);
    with_flag(sh.world > 1, [&](auto sharded) { hipLaunchKernelGGL((k_subj_expand<sharded()>), grid, dim3(kBlock), 0, st, s, f, iter, sh); });
}
void launch_subj_import_gathered(hipStream_t st, const DevSubjLevel &s, const DevFrontier &f, uint32_t iter, const uint4 *hdrs, const uint4 *data, uint32_t world,
                                 uint32_t rank, uint32_t cap, bool have_data, uint32_t *ctrl) {
    const uint32_t bx = import_gathered_blocks(cap, have_data);
    hipLaunchKernelGGL(k_subj_import_gathered, dim3(bx, world), dim3(256), 0, st, s, f, iter, hdrs, data, world, rank, cap, have_data ? 1u : 0u, ctrl);
}
void launch_subj_fold(hipStream_t st, const uint32_t *gathered, uint32_t world, uint32_t m, uint32_t row_words, uint32_t *out, uint32_t out_stride) {
    const size_t total = (size_t)m * out_stride;
    if (!total) return;
    hipLaunchKernelGGL(k_subj_fold, dim3((uint32_t)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0, st, gathered, world, m, row_words, out, out_stride);
}

// ---- watch sets: the records of new XOR old (kernels.hpp DevRowsDiff) ----
// Two passes over the rows so that the answer's order does not depend on which wave finishes first: the popcount of every tile, an exclusive scan of the
// tile counts, then every tile's wave writes its records where the scan says.  A wave walks its tile in steps of 256 words: lane l holds words
// 4 l .. 4 l + 3 of the step, so consecutive lanes hold consecutive bits and a wave prefix sum of the lanes' popcounts (DPP, wave_incl_scan) orders the records.
constexpr uint32_t kDiffStepWords = 256;  // 64 lanes x 4 words
static_assert(kDiffTileWords % kDiffStepWords == 0, "a tile is whole steps");

// words w0 .. w0 + 3 of a row of `width` words (w0 a multiple of 4); words from `width` on read as zero
template <bool VEC>
__device__ __forceinline__ uint4 diff_load4(const uint32_t *__restrict__ row, uint32_t width, uint32_t w0) {
    if (VEC) return w0 < width ? *reinterpret_cast<const uint4 *>(row + w0) : make_uint4(0u, 0u, 0u, 0u);  // (width is a multiple of 4: inside or outside as a whole)
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (w0 < width) v.x = row[w0];
    if (w0 + 1u < width) v.y = row[w0 + 1u];
    if (w0 + 2u < width) v.z = row[w0 + 2u];
    if (w0 + 3u < width) v.w = row[w0 + 3u];
    return v;
}
struct DiffTile {
    const uint32_t *orow, *nrow;
    uint32_t owidth, row, w_begin, w_end;
};
__device__ __forceinline__ DiffTile diff_tile(const DevRowsDiff &d, uint32_t ntiles, uint64_t t) {
    DiffTile x;
    x.row = (uint32_t)(t / ntiles);
    const uint32_t tile = (uint32_t)(t - (uint64_t)x.row * ntiles);
    x.owidth = x.row < d.old_nrows ? d.old_words : 0u;  // (a row the old array does not have: empty)
    x.orow = d.old_rows + (size_t)x.row * d.old_words;
    x.nrow = d.new_rows + (size_t)x.row * d.new_words;
    x.w_begin = tile * kDiffTileWords;
    x.w_end = min(x.w_begin + kDiffTileWords, max(d.old_words, d.new_words));
    return x;
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_rows_diff_count(DevRowsDiff d, uint32_t ntiles, uint32_t *__restrict__ tile_counts) {
    const uint32_t lane = lane_id();
    const uint64_t total = (uint64_t)ntiles * d.n_rows;
    for (uint64_t t = (uint64_t)blockIdx.x * 4u + uniform(threadIdx.x >> 6); t < total; t += (uint64_t)gridDim.x * 4u) {
        const DiffTile x = diff_tile(d, ntiles, t);
        uint32_t cnt = 0;
        if (!d.row_ids || d.row_ids[x.row] != kDiffSkipRow)
            for (uint32_t w0 = x.w_begin + lane * 4u; w0 < x.w_end; w0 += kDiffStepWords) {
                const uint4 a = diff_load4<VEC>(x.orow, x.owidth, w0), b = diff_load4<VEC>(x.nrow, d.new_words, w0);
                cnt += __popc(a.x ^ b.x) + __popc(a.y ^ b.y) + __popc(a.z ^ b.z) + __popc(a.w ^ b.w);
            }
        const uint32_t sum = wave_last(wave_incl_scan(cnt, 0u));
        if (lane == 0) tile_counts[t] = sum;
    }
}

// one block: offs[i] = counts[0] + ... + counts[i - 1], offs[n] = the total.  1024 counts per trip: a DPP scan per wave, the sixteen wave totals through LDS.
// (A tile holds at most 2^17 records, a trip at most 2^27: 32-bit sums inside a trip, the carry between trips is 64-bit.)
__global__ __launch_bounds__(1024) void k_rows_diff_scan(const uint32_t *__restrict__ counts, uint64_t n, unsigned long long *__restrict__ offs) {
    __shared__ uint32_t s_wave[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    unsigned long long carry = 0;
    for (uint64_t base = 0; base < n; base += 1024u) {
        const uint64_t i = base + tid;
        const uint32_t v = i < n ? counts[i] : 0u;
        const uint32_t incl = wave_incl_scan(v, 0u);
        if (lane == 63u) s_wave[wv] = incl;
        __syncthreads();
        uint32_t below = 0, all = 0;
#pragma unroll
        for (uint32_t k = 0; k < 16u; k++) {
            const uint32_t s = s_wave[k];
            all += s;
            if (k < wv) below += s;
        }
        if (i < n) offs[i] = carry + below + (incl - v);
        carry += all;
        __syncthreads();
    }
    if (tid == 0) offs[n] = carry;
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_rows_diff_emit(DevRowsDiff d, uint32_t ntiles, const unsigned long long *__restrict__ offs, uint4 *__restrict__ out,
                                                        unsigned long long out_cap) {
    const uint32_t lane = lane_id();
    const uint64_t total = (uint64_t)ntiles * d.n_rows;
    for (uint64_t t = (uint64_t)blockIdx.x * 4u + uniform(threadIdx.x >> 6); t < total; t += (uint64_t)gridDim.x * 4u) {
        unsigned long long base = offs[t];
        if (offs[t + 1] == base) continue;  // (nothing changed in this tile: the usual case, and what a skipped row looks like)
        const DiffTile x = diff_tile(d, ntiles, t);
        const uint32_t who = d.row_ids ? d.row_ids[x.row] : x.row;
        for (uint32_t ws = x.w_begin; ws < x.w_end; ws += kDiffStepWords) {  // (wave-uniform trip count: the prefix sum needs every lane)
            const uint32_t w0 = ws + lane * 4u;
            const uint4 a = diff_load4<VEC>(x.orow, x.owidth, w0), b = diff_load4<VEC>(x.nrow, d.new_words, w0);
            const uint32_t nw[4] = {b.x, b.y, b.z, b.w};
            uint32_t xw[4] = {a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w};
            const uint32_t cnt = __popc(xw[0]) + __popc(xw[1]) + __popc(xw[2]) + __popc(xw[3]);
            const uint32_t incl = wave_incl_scan(cnt, 0u);
            unsigned long long pos = base + (incl - cnt);
            base += wave_last(incl);
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++)
                for (uint32_t m = xw[k]; m; m &= m - 1u) {
                    const uint32_t bit = (uint32_t)__ffs((int)m) - 1u;
                    if (pos < out_cap) out[pos] = make_uint4(who, (w0 + k) * 32u + bit, (nw[k] >> bit) & 1u, 0u);
                    pos++;
                }
        }
    }
}

static uint32_t rows_diff_blocks(uint64_t tiles) { return (uint32_t)std::min<uint64_t>((tiles + 3) / 4, 4096); }
static bool rows_diff_vec(const DevRowsDiff &d) { return d.old_words % 4u == 0 && d.new_words % 4u == 0; }
void launch_rows_diff_count(hipStream_t st, const DevRowsDiff &d, uint32_t *tile_counts, uint64_t *offs) {
    const uint32_t ntiles = rows_diff_tiles(d);
    const uint64_t tiles = (uint64_t)ntiles * d.n_rows;
    if (tiles)
        with_flag(rows_diff_vec(d), [&](auto vec) { hipLaunchKernelGGL((k_rows_diff_count<vec()>), dim3(rows_diff_blocks(tiles)), dim3(256), 0, st, d, ntiles, tile_counts); });
    hipLaunchKernelGGL(k_rows_diff_scan, dim3(1), dim3(1024), 0, st, tile_counts, tiles, (unsigned long long *)offs);
}
void launch_rows_diff_emit(hipStream_t st, const DevRowsDiff &d, const uint64_t *offs, uint4 *out, uint64_t out_cap) {
    const uint32_t ntiles = rows_diff_tiles(d);
    const uint64_t tiles = (uint64_t)ntiles * d.n_rows;
    if (!tiles || !out_cap) return;
    with_flag(rows_diff_vec(d), [&](auto vec) {
        hipLaunchKernelGGL((k_rows_diff_emit<vec()>), dim3(rows_diff_blocks(tiles)), dim3(256), 0, st, d, ntiles, (const unsigned long long *)offs, out, (unsigned long long)out_cap);
    });
}

// ---- lookup cursors: pages of ids out of rows kept on the device (kernels.hpp DevRowsPage) ----
// The rank index is the diff's own count + scan against an empty old array: offs[row * ntiles + tile] = set bits in front of the tile, over all rows.
// plan: one wave per request.  start = after_id + 1 (ACL_PAGE_FROM_START wraps to 0); rank0 = the index's offset of the start's tile + the popcount of the
//       tile's bits below start; rank_end = min(rank0 + limit, the row's end rank).  Leaves {rank0, rank_end} for the emit and n | more << 31 for the host.
// page: one wave per (request, tile).  The tile's rank interval [offs[t], offs[t + 1]) against [rank0, rank_end) decides whether the wave has anything to
//       do; a live wave walks its tile as k_rows_diff_emit does and writes the id of every set bit whose rank is in range at ids[base + rank - rank0].
//       Where an id lands depends on its rank alone: no atomics, no order between waves.
__global__ __launch_bounds__(256) void k_rows_page_plan(DevRowsPage p, const uint4 *__restrict__ reqs, uint32_t m, ulonglong2 *__restrict__ plan, uint32_t *__restrict__ res) {
    const uint32_t lane = lane_id();
    for (uint32_t q = blockIdx.x * 4u + uniform(threadIdx.x >> 6); q < m; q += gridDim.x * 4u) {
        const uint4 rq = reqs[q];  // {row, after_id, limit, base}
        const uint32_t row = rq.x, start = rq.y + 1u;
        const unsigned long long *ro = (const unsigned long long *)p.offs + (size_t)row * p.ntiles;
        const unsigned long long row_end = ro[p.ntiles];
        unsigned long long rank0 = row_end;
        if (start < p.row_words * 32ull) {  // (wave-uniform: the request's own words)
            const uint32_t t0 = start / (kDiffTileWords * 32u), sw = start >> 5, smask = (1u << (start & 31u)) - 1u;
            const uint32_t *r = p.rows + (size_t)row * p.row_words;
            uint32_t cnt = 0;
            for (uint32_t w0 = t0 * kDiffTileWords + lane * 4u; w0 <= sw; w0 += kDiffStepWords) {  // (w0 <= sw < row_words, both multiples of 4 apart from sw: the load is inside the row)
                const uint4 v = *reinterpret_cast<const uint4 *>(r + w0);
                const uint32_t x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (uint32_t k = 0; k < 4u; k++) cnt += __popc(w0 + k < sw ? x[k] : (w0 + k == sw ? x[k] & smask : 0u));
            }
            rank0 = ro[t0] + wave_last(wave_incl_scan(cnt, 0u));
        }
        const unsigned long long rank_end = min(rank0 + rq.z, row_end);
        if (lane == 0) {
            plan[q] = make_ulonglong2(rank0, rank_end);
            res[q] = (uint32_t)(rank_end - rank0) | (row_end > rank_end ? 0x80000000u : 0u);
        }
    }
}

__global__ __launch_bounds__(256) void k_rows_page(DevRowsPage p, const uint4 *__restrict__ reqs, uint32_t m, const ulonglong2 *__restrict__ plan, uint32_t *__restrict__ ids) {
    const uint32_t lane = lane_id();
    const uint64_t total = (uint64_t)p.ntiles * m;
    for (uint64_t t = (uint64_t)blockIdx.x * 4u + uniform(threadIdx.x >> 6); t < total; t += (uint64_t)gridDim.x * 4u) {
        const uint32_t q = (uint32_t)(t / p.ntiles), tile = (uint32_t)(t - (uint64_t)q * p.ntiles);
        const ulonglong2 pl = plan[q];
        const unsigned long long rank0 = pl.x, rank_end = pl.y;
        if (rank0 >= rank_end) continue;
        const uint4 rq = reqs[q];
        const unsigned long long *ro = (const unsigned long long *)p.offs + (size_t)rq.x * p.ntiles + tile;
        unsigned long long base = ro[0];
        if (base >= rank_end || ro[1] <= rank0) continue;  // (the tile's ranks do not meet the page's: most waves leave here)
        const uint32_t *r = p.rows + (size_t)rq.x * p.row_words;
        uint32_t *out = ids + rq.w;
        const uint32_t w_begin = tile * kDiffTileWords, w_end = min(w_begin + kDiffTileWords, p.row_words);
        for (uint32_t ws = w_begin; ws < w_end && base < rank_end; ws += kDiffStepWords) {  // (wave-uniform trip count: the prefix sum needs every lane)
            const uint32_t w0 = ws + lane * 4u;
            const uint4 v = diff_load4<true>(r, p.row_words, w0);
            const uint32_t xw[4] = {v.x, v.y, v.z, v.w};
            const uint32_t cnt = __popc(xw[0]) + __popc(xw[1]) + __popc(xw[2]) + __popc(xw[3]);
            const uint32_t incl = wave_incl_scan(cnt, 0u);
            unsigned long long pos = base + (incl - cnt);
            base += wave_last(incl);
            if (pos + cnt > rank0 && pos < rank_end) {  // (else: this lane's bits lie outside the page)
#pragma unroll
                for (uint32_t k = 0; k < 4u; k++)
                    for (uint32_t mm = xw[k]; mm; mm &= mm - 1u) {
                        if (pos >= rank0 && pos < rank_end) out[pos - rank0] = (w0 + k) * 32u + (uint32_t)__ffs((int)mm) - 1u;  // (pos - rank0 < limit: inside the request's own slice of ids)
                        pos++;
                    }
            }
        }
    }
}

void launch_rows_page(hipStream_t st, const DevRowsPage &p, const uint4 *reqs, uint32_t m, void *plan, uint32_t *res, uint32_t *ids) {
    if (!m) return;
    hipLaunchKernelGGL(k_rows_page_plan, dim3(std::min<uint32_t>((m + 3u) / 4u, 4096u)), dim3(256), 0, st, p, reqs, m, (ulonglong2 *)plan, res);
    hipLaunchKernelGGL(k_rows_page, dim3(rows_diff_blocks((uint64_t)p.ntiles * m)), dim3(256), 0, st, p, reqs, m, (const ulonglong2 *)plan, ids);
}

// ---- derived lookup cursors: rows that are boolean combinations of rows kept on the device (kernels.hpp DevRowsDerive) ----
// One wave per (expression, tile), walked as k_rows_diff_count walks its tile: per step a lane holds 4 words of the result.  The wave's expression and tile
// are made uniform (readfirstlane), so the expression record and the operand records {row base, words} come by scalar loads and every lane of a step loads
// from the same operand row.  A lane whose words lie behind an operand's width takes zero for it and does not load.  The result is stored once (not in count
// mode), its popcount is reduced over the wave and left in tile_counts[expr * ntiles + tile] by one lane: no atomics, no LDS, no order between waves.
// "Everything" (an empty any-list) is the start value of the AND over the all-list, which is never empty then -- so bits behind the type's last id, zero in
// every operand, stay zero.
__device__ __forceinline__ uint4 derive_load4(const ulonglong2 op, uint32_t w0) {  // op: {row base, words (a multiple of 4) in the low half of y}
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef const u32x4 __attribute__((address_space(1))) * global_u32x4;  // (an address out of a record: say that it is global memory, else the load is a flat one)
    if (w0 >= (uint32_t)op.y) return make_uint4(0u, 0u, 0u, 0u);
    const u32x4 v = *(global_u32x4)(op.x + (unsigned long long)w0 * 4u);
    return make_uint4(v.x, v.y, v.z, v.w);
}
// folds the n operand rows ops[0 .. n) into r at words w0 .. w0 + 3 -- MODE 0: r |= v, 1: r &= v, 2: r &= ~v.  Four operands per trip: their loads are issued
// together (the list's length is wave-uniform, so is every guard; a guard that fails stands in the fold's neutral value and reads no record)
template <int MODE>
__device__ __forceinline__ void derive_fold(uint4 &r, const ulonglong2 *__restrict__ ops, uint32_t n, uint32_t w0) {
    const uint32_t neutral = MODE == 1 ? 0xFFFFFFFFu : 0u;
    for (uint32_t k = 0; k < n; k += 4u) {
        uint4 v[4];
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++) v[j] = k + j < n ? derive_load4(ops[k + j], w0) : make_uint4(neutral, neutral, neutral, neutral);
        issue_fence();
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++) {
            if (MODE == 0) r.x |= v[j].x, r.y |= v[j].y, r.z |= v[j].z, r.w |= v[j].w;
            if (MODE == 1) r.x &= v[j].x, r.y &= v[j].y, r.z &= v[j].z, r.w &= v[j].w;
            if (MODE == 2) r.x &= ~v[j].x, r.y &= ~v[j].y, r.z &= ~v[j].z, r.w &= ~v[j].w;
        }
    }
}
__global__ __launch_bounds__(256) void k_rows_derive(const uint4 *__restrict__ exprs, const ulonglong2 *__restrict__ ops, uint32_t *__restrict__ out, uint32_t out_words,
                                                     uint32_t ntiles, uint32_t n_exprs, uint32_t *__restrict__ tile_counts) {
    const uint32_t lane = lane_id();
    const uint64_t total = (uint64_t)ntiles * n_exprs;
    for (uint64_t t = (uint64_t)blockIdx.x * 4u + uniform(threadIdx.x >> 6); t < total; t += (uint64_t)gridDim.x * 4u) {
        const uint32_t e = uniform((uint32_t)(t / ntiles)), tile = uniform((uint32_t)(t - (uint64_t)e * ntiles));
        const uint4 x = exprs[e];  // {first, n_any, n_all, n_none}
        const ulonglong2 *any = ops + x.x, *all = any + x.y, *none = all + x.z;
        const uint32_t w_begin = tile * kDiffTileWords, w_end = min(w_begin + kDiffTileWords, out_words);
        uint32_t cnt = 0;
        for (uint32_t w0 = w_begin + lane * 4u; w0 < w_end; w0 += kDiffStepWords) {
            const uint32_t init = x.y ? 0u : 0xFFFFFFFFu;  // (no any-list: "everything", cut down by the all-list, which is not empty then)
            uint4 r = make_uint4(init, init, init, init);
            derive_fold<0>(r, any, x.y, w0);
            derive_fold<1>(r, all, x.z, w0);
            derive_fold<2>(r, none, x.w, w0);
            if (out) *reinterpret_cast<uint4 *>(out + (size_t)e * out_words + w0) = r;  // (w0 + 3 < w_end <= out_words: inside the expression's own row)
            cnt += __popc(r.x) + __popc(r.y) + __popc(r.z) + __popc(r.w);
        }
        const uint32_t sum = wave_last(wave_incl_scan(cnt, 0u));
        if (lane == 0) tile_counts[t] = sum;
    }
}

void launch_rows_derive(hipStream_t st, const DevRowsDerive &d, uint32_t *tile_counts, uint64_t *offs) {
    const uint64_t tiles = (uint64_t)d.ntiles * d.n_exprs;
    if (!tiles) return;
    hipLaunchKernelGGL(k_rows_derive, dim3(rows_diff_blocks(tiles)), dim3(256), 0, st, (const uint4 *)d.exprs, (const ulonglong2 *)d.ops, d.out, d.out_words, d.ntiles, d.n_exprs,
                       tile_counts);
    hipLaunchKernelGGL(k_rows_diff_scan, dim3(1), dim3(1024), 0, st, tile_counts, tiles, (unsigned long long *)offs);
}

// ---- subject-direction watch sets: the candidates of a non-monotone permission confirmed where the rows are (kernels.hpp DevRefine) ----
// The candidate records are the diff's own (rows against an empty old array: one {row, bit, 1, 0} per set bit, ordered by (row, bit)); the stand-ins
// of the flagged rows follow them.  Item k answers record k, so k_refine_apply needs no search: lanes of a wave hold consecutive records, the ones
// that share a row word are neighbours and fold their bits before the one atomic (subj_mark's fold, with AND NOT in the place of OR).

// the rows in `wrows`: bits [0, nobj) set, the wildcard's own bit (wid < nobj) cleared; one word per thread
__global__ __launch_bounds__(256) void k_refine_fill(DevRefine r, uint32_t nflag, uint32_t need, uint32_t nobj, uint32_t wid) {
    const uint64_t total = (uint64_t)nflag * need;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256u) {
        const uint32_t f = (uint32_t)(i / need), w = (uint32_t)(i - (uint64_t)f * need);
        uint32_t v = w * 32u + 32u <= nobj ? 0xFFFFFFFFu : (1u << (nobj & 31u)) - 1u;  // (need = ceil(nobj / 32): only the last word is partial)
        if (wid < nobj && (wid >> 5) == w) v &= ~(1u << (wid & 31u));
        r.rows[(size_t)r.wrows[f] * r.row_words + w] = v;
    }
}

// rows whose flag word is raised: the wildcard's bit set (every row has one thread: a plain read-modify-write)
__global__ __launch_bounds__(256) void k_refine_wild(uint32_t *rows, uint32_t row_words, const uint32_t *__restrict__ flags, uint32_t n_rows, uint32_t wid) {
    const uint32_t row = blockIdx.x * 256u + threadIdx.x;
    if (row < n_rows && flags[row]) rows[(size_t)row * row_words + (wid >> 5)] |= 1u << (wid & 31u);
}

__global__ __launch_bounds__(256) void k_refine_items(DevRefine r, uint4 *__restrict__ items) {
    const uint32_t n = r.nrec + r.nstand;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        uint32_t row, sid;
        if (i < r.nrec) {
            const uint4 rec = r.recs[i];  // {row of the slice, bit, 1, 0}
            row = r.row0 + rec.x;
            sid = rec.y;
        } else {
            row = r.wrows[r.wrow0 + (i - r.nrec)];
            sid = r.fresh_sid;
        }
        items[i] = make_uint4(r.head, r.rids[row], r.tail, sid);  // acl_item_t: {type | permission << 16, resource, subject type | relation << 16, subject}
    }
}

__global__ __launch_bounds__(256) void k_refine_apply(DevRefine r, const uint8_t *__restrict__ perm, const int32_t *__restrict__ err, uint32_t has_value, uint32_t *status) {
    const uint32_t lane = lane_id(), n = r.nrec + r.nstand;
    for (uint32_t base = (blockIdx.x * 4u + uniform(threadIdx.x >> 6)) * 64u; base < n; base += gridDim.x * 256u) {  // (wave-uniform trips: the fold shuffles)
        const uint32_t i = base + lane;
        const bool in = i < n, is_rec = i < r.nrec;
        const bool bad = in && err[i] != 0;
        const bool holds = in && !bad && perm[i] == has_value;
        uint32_t w = 0xFFFFFFFFu, b = 0u;
        if (is_rec) {
            const uint4 rec = r.recs[i];
            w = (r.row0 + rec.x) * r.row_words + (rec.y >> 5);  // (a set's rows are below 2^28 words)
            b = holds ? 0u : 1u << (rec.y & 31u);
        } else if (in) {
            r.flags[r.wrows[r.wrow0 + (i - r.nrec)]] = holds ? 1u : 0u;  // the stand-in decides the row's wildcard
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t ow = (uint32_t)__shfl_down((int)w, d), ob = (uint32_t)__shfl_down((int)b, d);
            if (lane + (uint32_t)d < 64u && ow == w) b |= ob;
        }
        const uint32_t pw = (uint32_t)__shfl_up((int)w, 1);
        if (is_rec && b && (lane == 0u || pw != w)) __hip_atomic_fetch_and(r.rows + w, ~b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long errs = __ballot(bad);
        if (errs && lane == (uint32_t)__ffsll((long long)errs) - 1u) __hip_atomic_fetch_min(status, i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // the wave's first erring item
    }
}

// dst[row][0 .. dst_words) = src[row][0 .. src_words) followed by zeros, dst_flags[row] = src_flags[row]: the walk's packed rows into a set's row array
__global__ __launch_bounds__(256) void k_subj_rows_store(const uint32_t *__restrict__ src, uint32_t src_words, const uint32_t *__restrict__ src_flags, uint32_t m, uint32_t *__restrict__ dst,
                                                         uint32_t dst_words, uint32_t *__restrict__ dst_flags) {
    const uint64_t total = (uint64_t)m * dst_words;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256u) {
        const uint32_t row = (uint32_t)(i / dst_words), w = (uint32_t)(i - (uint64_t)row * dst_words);
        dst[i] = w < src_words ? src[(size_t)row * src_words + w] : 0u;
        if (w == 0u) dst_flags[row] = src_flags[row];
    }
}

// ---- Explain proofs: a round's candidates become items and their answers are folded per goal on the device (kernels.hpp DevProofPick) ----
__global__ __launch_bounds__(256) void k_proof_items(DevProofPick p, uint4 *__restrict__ items) {
    for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < p.ncand; k += gridDim.x * 256u) {
        const uint32_t g = p.group[k];
        // (a group index the host did not hand out names no header: the item is left ill-formed on purpose -- type 0xFFFF -- and answers with an error)
        const uint4 gr = g < p.ngroups ? p.groups[g] : make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u);
        items[k] = make_uint4(gr.x, p.obj[k], gr.y, gr.z);  // acl_item_t: {type | permission << 16, resource, subject type | relation << 16, subject}
    }
}

__global__ __launch_bounds__(256) void k_proof_rows(DevProofRows r) {
    __shared__ uint32_t s_at, s_deg, s_first;
    const uint2 *__restrict__ meta2 = reinterpret_cast<const uint2 *>(r.meta);
    for (uint32_t g = blockIdx.x; g < r.ngroups; g += gridDim.x) {  // (block-uniform trips: the barriers)
        if (threadIdx.x == 0) {
            const uint2 rw = r.rows[g];
            uint32_t at = 0, deg = 0, first = 0;
            if (rw.x < r.meta_pairs) {
                const uint2 md = meta2[rw.x];
                if (md.y > md.x && md.y <= r.nedges && md.y - md.x > rw.y) {
                    first = md.x + rw.y;
                    deg = md.y - first;
                    const unsigned long long was = __hip_atomic_fetch_add(reinterpret_cast<unsigned long long *>(r.total), (unsigned long long)deg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (was + deg > (unsigned long long)r.cap) {  // the region is full: the caller redoes the pass with a larger one
                        __hip_atomic_fetch_or(r.total + 2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        deg = 0;
                    } else {
                        at = (uint32_t)was;
                    }
                }
                r.groups[g].w = at;
                r.gn[g] = deg;
            }
            s_at = at;
            s_deg = deg;
            s_first = first;
        }
        __syncthreads();
        const uint32_t at = s_at, deg = s_deg, first = s_first;
        for (uint32_t i = threadIdx.x; i < deg; i += 256u) {  // (at + deg <= cap and first + deg <= nedges were checked by thread 0)
            r.obj[at + i] = r.edges[first + i] & kIdMask;
            r.group[at + i] = g;
        }
        __syncthreads();  // (before thread 0 overwrites the three words for the block's next group)
    }
}

__global__ __launch_bounds__(256) void k_proof_winner(DevProofPick p, uint32_t *__restrict__ win) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < 2u * p.ngroups; i += gridDim.x * 256u) {
        const uint32_t f = p.first[i];
        const uint64_t at = (uint64_t)p.groups[i >> 1].w + f;
        win[i] = (f != 0xFFFFFFFFu && at < p.ncand) ? p.obj[at] : 0xFFFFFFFFu;
    }
}

__global__ __launch_bounds__(256) void k_proof_pick(DevProofPick p, const uint8_t *__restrict__ perm, const int32_t *__restrict__ err, uint32_t has_value, uint32_t no_value) {
    const uint32_t lane = lane_id();
    for (uint32_t base = (blockIdx.x * 4u + uniform(threadIdx.x >> 6)) * 64u; base < p.ncand; base += gridDim.x * 256u) {  // (wave-uniform trips: the ballots)
        const uint32_t k = base + lane;
        uint32_t g = 0xFFFFFFFFu;
        bool has = false, no = false;
        if (k < p.ncand) {
            g = p.group[k];
            if (g < p.ngroups) {
                const bool clean = err[k] == 0;
                const uint32_t v = perm[k];
                has = clean && v == has_value;
                no = clean && v == no_value;
            } else {
                g = 0xFFFFFFFFu;
            }
        }
        const uint32_t g0 = uniform(g);  // lane 0 is in range (base < ncand)
        if (!__ballot(g != g0 && g != 0xFFFFFFFFu)) {  // one group in the wave (lanes behind the end, if any, carry none): one lane speaks for all
            if (g0 == 0xFFFFFFFFu) continue;
            const unsigned long long hb = __ballot(has), nb = __ballot(no);
            if (lane == 0u) {
                const uint32_t at = base - p.groups[g0].w;  // lane 0's index inside the group
                if (hb) {
                    __hip_atomic_fetch_min(p.first + 2u * g0, at + (uint32_t)__ffsll((long long)hb) - 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_fetch_add(p.count + 2u * g0, (uint32_t)__popcll(hb), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                if (nb) {
                    __hip_atomic_fetch_min(p.first + 2u * g0 + 1u, at + (uint32_t)__ffsll((long long)nb) - 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_fetch_add(p.count + 2u * g0 + 1u, (uint32_t)__popcll(nb), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        } else if (has || no) {  // a wave that spans groups: every answering lane for itself
            const uint32_t at = k - p.groups[g].w, w = 2u * g + (no ? 1u : 0u);
            __hip_atomic_fetch_min(p.first + w, at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(p.count + w, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

static uint32_t refine_blocks(uint64_t threads) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((threads + 255) / 256, 4096)); }
void launch_proof_items(hipStream_t st, const DevProofPick &p, uint4 *items) {
    if (!p.ncand || !p.ngroups) return;
    hipLaunchKernelGGL(k_proof_items, dim3(refine_blocks(p.ncand)), dim3(256), 0, st, p, items);
}
void launch_proof_rows(hipStream_t st, const DevProofRows &r) {
    if (!r.ngroups) return;
    hipLaunchKernelGGL(k_proof_rows, dim3(std::min<uint32_t>(r.ngroups, 4096u)), dim3(256), 0, st, r);
}
void launch_proof_winner(hipStream_t st, const DevProofPick &p, uint32_t *win) {
    if (!p.ngroups) return;
    hipLaunchKernelGGL(k_proof_winner, dim3(refine_blocks(2ull * p.ngroups)), dim3(256), 0, st, p, win);
}
void launch_proof_pick(hipStream_t st, const DevProofPick &p, const uint8_t *perm, const int32_t *err, uint32_t has_value, uint32_t no_value) {
    if (!p.ncand || !p.ngroups) return;
    hipLaunchKernelGGL(k_proof_pick, dim3(refine_blocks(p.ncand)), dim3(256), 0, st, p, perm, err, has_value, no_value);
}
void launch_subj_rows_store(hipStream_t st, const uint32_t *src, uint32_t src_words, const uint32_t *src_flags, uint32_t m, uint32_t *dst, uint32_t dst_words, uint32_t *dst_flags) {
    if (!m || !dst_words) return;
    hipLaunchKernelGGL(k_subj_rows_store, dim3(refine_blocks((uint64_t)m * dst_words)), dim3(256), 0, st, src, src_words, src_flags, m, dst, dst_words, dst_flags);
}
void launch_refine_fill(hipStream_t st, const DevRefine &r, uint32_t nflag, uint32_t need, uint32_t nobj, uint32_t wid) {
    if (!nflag || !need) return;
    hipLaunchKernelGGL(k_refine_fill, dim3(refine_blocks((uint64_t)nflag * need)), dim3(256), 0, st, r, nflag, need, nobj, wid);
}
void launch_refine_wild(hipStream_t st, uint32_t *rows, uint32_t row_words, const uint32_t *flags, uint32_t n_rows, uint32_t wid) {
    if (!n_rows || (wid >> 5) >= row_words) return;
    hipLaunchKernelGGL(k_refine_wild, dim3((n_rows + 255) / 256), dim3(256), 0, st, rows, row_words, flags, n_rows, wid);
}
void launch_refine_items(hipStream_t st, const DevRefine &r, uint4 *items) {
    if (!(r.nrec + r.nstand)) return;
    hipLaunchKernelGGL(k_refine_items, dim3(refine_blocks(r.nrec + r.nstand)), dim3(256), 0, st, r, items);
}
void launch_refine_apply(hipStream_t st, const DevRefine &r, const uint8_t *perm, const int32_t *err, uint32_t has_value, uint32_t *status) {
    if (!(r.nrec + r.nstand)) return;
    hipLaunchKernelGGL(k_refine_apply, dim3(refine_blocks(r.nrec + r.nstand)), dim3(256), 0, st, r, perm, err, has_value, status);
}

}  // namespace acl

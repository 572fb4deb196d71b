// engine_keep.cpp -- PostFilter and CheckBulkPermissions for ONE subject by the reverse walk: the depth sweep that makes the pair
// form sound, the route itself, its K x F form, and the keep / packed entry points that try it before the forward path.
#include "engine_strings.hpp"

namespace aclint {

// ---- the route's thresholds
constexpr size_t kRouteMinPairs = 512;  // fewer pairs go forward (ACL_KEEP_ROUTE_MIN overrides: A/B and test knob; 0 switches the route off)
// FEW allowed objects: so few that hashing THEIR names (a dependent miss or three each: id -> name -> bytes) is cheaper than sending the call's names to the
// table -- a thirty-second of the pairs (a power user with 10 000 allowed pods among 65 536 pairs took 0.32 ms through the tags, 0.13 through the table)
constexpr uint64_t kFewFloor = 64, kFewShare = 32;
// a short list for a far-reaching subject goes forward (KeepCall::prepare): reach from 4 096 objects, lists below 8 192 pairs, every 16th call walks anyway
constexpr uint64_t kShortListReach = 4096;
constexpr size_t kShortListPairs = 8192;
constexpr uint32_t kShortListRetry = 15u;
// the pool takes the pass and the test from 2 048 items on, from 512 when its workers are still polling after the previous call (intern_items); the tags
// of fewer than 256 allowed objects are filled by the caller alone
constexpr size_t kSpreadMin = 2048, kSpreadHotMin = 512;
constexpr uint64_t kTagFillSpreadMin = 256;
constexpr size_t kPairBlock = 64;  // pairs per stage of the pass and of the test
// the depth sweep: a type of up to 2^20 objects, or 64 per pair of the call (a sweep of more than ~1 ms for a call that is not itself that long: forward)
constexpr size_t kSweepMaxObjects = (size_t)1 << 20, kSweepObjectsPerPair = 64;
// K x F (keep_by_reverse_walks): F = 2 ... 4 templates, from 512 items on; over a type of more than 262 144 objects from 16 384 items on (ACL_KEEP_MULTI_MIN overrides)
constexpr size_t kMultiMinTemplates = 2, kMultiMaxTemplates = 4, kMultiMinItems = 512, kMultiBigType = 262144, kMultiBigMinItems = 16384;

// ---- PostFilter by ONE reverse walk (round 6).  filterItemsWithBulkPermissions (reference pkg/authz/postfilter.go:58-182) resolves every
// template of every list item for the REQUESTING USER: K x F pairs that share their subject and, per template, type and permission.  K forward walks from K
// resources ask the graph the same question LookupResources answers once: which objects of the type may this subject see.  So when all pairs of a call share
// (resource type, permission, subject type, subject id) -- a plain subject, a permission whose value no `&` / `-` can change -- the engine runs the reverse
// walk once and tests the K resource names against its row.  For a subject with FEW allowed objects it tests them the cheap way round: the row's allowed
// objects give a small set of name-hash tags that stays in cache; a pair's resource name is hashed (no memory touched but its own bytes) and looked up THERE
// -- only a tag hit goes on to the type's name table for the id and the bit, and a name the user may not see never pays the table's miss.  With MANY allowed
// every name is resolved in the table -- by the host's pass over the pairs, while the device still walks.  Every deviation -- fields that differ, a userset subject, an item the API's validation
// would refuse, a non-monotone permission, a sharded or store-only engine -- returns kRouteNotTaken BEFORE anything is written, and the caller takes the
// forward path -- as does a subject no table knows while the store holds a `T:*` relationship of its type (without one it is answered "nothing is allowed"
// with no walk at all; with one, the wildcard's rows grant it what they grant everybody): keep mask and error behaviour are the forward path's by construction (an unknown or unreachable resource is NO_PERMISSION there, a depth
// error is a pair error there: both drop the item, postfilter.go:162-172, as the missing bit does here).
// "No Check of (rt, pm) for a subject of type st ends at the dispatch-depth limit on this snapshot" -- what lets the PAIR form below answer a RECURSIVE permission
// (nested groups: the schema alone allows a chain of any length) from the reverse walk's row.  A Check that does not find its subject explores every path below
// its resource, whoever the subject is (the oracle's and the kernels' rule: HAS_PERMISSION wins, else a path beyond the limit is the pair's error, else NO; no
// path's length depends on who is looked for), so the set of resources with a depth error is the set a subject NOBODY IS gets one for: one forward sweep over the
// type's ids with the unknown-subject id (what intern_check_item gives a name no table holds), through the ordinary walk.  "None is deep" then holds until a
// write ADDS a path (Store::path_adds: a userset subject, an arrow's tupleset, a bulk load -- a plain grant ends the paths it is on, a removal only takes paths
// away); "some object is deep" is remembered for its own snapshot epoch only (acl_engine::snap_epoch).  The sweep costs a forward pass over the whole type
// (845 000 pods: ~1 ms), so it is only run for a graph that holds still: the first call that needs it goes forward and leaves a note, the next one that finds
// the note current sweeps.
// true: known for this snapshot -- none is deep, or *deep_out holds the deep objects' bitmap; false: not known (yet): the caller takes the forward path (a sweep that
// fails is "not known").  Caller holds state_mu shared (an Eval) and owns context c.
// *deep_out: the deep objects' bitmap when there are some (the pair form then answers their depth error per pair), empty when none is deep.
static bool no_object_is_deep(acl_engine *h, PassCtx *c, int rt, int pm, int st, size_t n_pairs, std::shared_ptr<const std::vector<uint32_t>> *deep_out) {
    static const bool kOff = getenv("ACL_DEPTH_SWEEP") && atoi(getenv("ACL_DEPTH_SWEEP")) == 0;  // (A/B and test knob)
    if (kOff) return false;
    const uint64_t epoch = h->snap_epoch, adds = h->store.path_adds();  // (writers hold state_mu exclusive: both belong to the snapshot the caller evaluates)
    const size_t count = h->store.objects(rt).count();
    if (count > std::max<size_t>(kSweepMaxObjects, kSweepObjectsPerPair * n_pairs)) return false;  // (a sweep of more than ~1 ms for a call that is not itself that long: forward)
    {
        std::lock_guard<std::mutex> lk(h->deep_mu);
        acl_engine::DeepKnown *k = nullptr;
        for (auto &d : h->deep_known)
            if (d.rt == rt && d.pm == pm && d.st == st) k = &d;
        if (!k) {
            if (h->deep_known.size() >= 64) h->deep_known.erase(h->deep_known.begin());
            h->deep_known.push_back(acl_engine::DeepKnown{});
            k = &h->deep_known.back();
            k->rt = rt, k->pm = pm, k->st = st;
        }
        if (k->swept && k->none && k->adds == adds) return true;  // shallow when swept, and nothing written since could have added a path
        if (k->swept && k->epoch == epoch) {                      // (this very snapshot: deep objects were found -- here is which)
            *deep_out = k->bits;
            return true;
        }
        // not known for this snapshot.  The sweep is for a graph that holds still: the first call that needs it leaves a note and goes forward, the next one
        // that finds the note still current sweeps -- current by the store's path_adds (plain grants and removals come and go without touching it), or, after a
        // sweep that FOUND deep objects, by the snapshot's epoch (only a removal can help then, and any write may be one)
        static const bool kEager = getenv("ACL_DEPTH_SWEEP") && atoi(getenv("ACL_DEPTH_SWEEP")) == 2;  // (tests: sweep at the first call)
        const bool by_epoch = k->swept && !k->none && k->adds == adds;
        const uint64_t key = by_epoch ? epoch : adds;
        if ((k->wanted != key || k->wanted_by_epoch != by_epoch) && !kEager) {
            k->wanted = key;
            k->wanted_by_epoch = by_epoch;
            return false;
        }
    }
    // (two callers may sweep the same epoch side by side: same answer, stored twice)
    const size_t chunk = std::min<size_t>(std::max<size_t>(h->max_sub_batch, 1), 262144);
    std::vector<acl_item_t> items(std::min(chunk, std::max<size_t>(count, 1)));
    std::vector<uint8_t> perm(items.size());
    std::vector<int32_t> err(items.size());
    bool none = true;
    auto bits = std::make_shared<std::vector<uint32_t>>();
    for (size_t b = 0; b < count; b += chunk) {
        const size_t m = std::min(chunk, count - b);
        for (size_t i = 0; i < m; i++) items[i] = acl_item_t{(uint16_t)rt, (uint16_t)pm, (uint32_t)(b + i), (uint16_t)st, (uint16_t)ACL_NO_RELATION, 0xFFFFFFFCu};
        if (check_ids_host(h, c, items.data(), m, perm.data(), err.data())) return false;
        for (size_t i = 0; i < m; i++)
            if (err[i]) {  // (any error is the depth error: an invalid item cannot happen -- the ids are the type's own)
                if (none) bits->assign((count + 31) / 32, 0u);
                none = false;
                (*bits)[(b + i) >> 5] |= 1u << ((b + i) & 31u);
            }
    }
    h->depth_sweeps.fetch_add(1, std::memory_order_relaxed);
    std::lock_guard<std::mutex> lk(h->deep_mu);
    for (auto &d : h->deep_known)
        if (d.rt == rt && d.pm == pm && d.st == st) {
            d.swept = true;
            d.none = none;
            d.epoch = epoch;
            d.adds = adds;
            d.bits = none ? nullptr : bits;
        }
    if (!none) *deep_out = bits;
    return true;
}

namespace {  // (the route's own types: nothing of them leaves this file)

// "Are the five constant fields of pair i those of pair 0?" -- the sample before any lock is taken and the pass over every pair ask the same question.
template <class Items>
static inline bool same_constants(const Items &its, size_t i) {
    static const int kConst[5] = {F_RT, F_PM, F_ST, F_SID, F_SR};
    // (the usual case first: the shim points every pair's constant fields at the same strings / dictionary entries -- no bytes compared)
    bool same = true, identical = false;
    if constexpr (std::is_same_v<Items, PackedItems>) {
        const uint32_t *x = its.rq->items + 6 * i, *y = its.rq->items;
        identical = ((x[F_RT] ^ y[F_RT]) | (x[F_PM] ^ y[F_PM]) | (x[F_ST] ^ y[F_ST]) | (x[F_SID] ^ y[F_SID]) | (x[F_SR] ^ y[F_SR])) == 0;
    } else if constexpr (std::is_same_v<Items, ViewItems>) {
        const auto *x = &its.it[i].resource_type, *y = &its.it[0].resource_type;
        identical = true;
        for (int k = 0; k < 5; k++) identical &= x[kConst[k]].p == y[kConst[k]].p && x[kConst[k]].n == y[kConst[k]].n;
    }
    for (int k = 0; k < 5 && same && !identical; k++) {
        const int f = kConst[k];
        const char *x = its.ptr(i, f), *y = its.ptr(0, f);
        const size_t lx = its.len(i, f), ly = its.len(0, f);
        same = lx == ly && (x == y || (x && y && std::memcmp(x, y, lx) == 0) || (lx == 0 && (!x || !y)));
    }
    return same;
}

// The allowed objects' name tags: open addressing over the upper half of the names' hashes (0 = empty; a tag of 0 is stored as 1: only costs a rare extra probe).
struct TagSet {
    std::vector<uint32_t> slots;
    uint32_t mask = 0;
    static uint32_t tag_of(uint64_t hash) {
        const uint32_t tg = (uint32_t)(hash >> 32);
        return tg + (tg == 0u);
    }
    void reset(uint64_t count) {
        size_t cap = 64;
        while (cap < 2 * count) cap <<= 1;
        slots.assign(cap, 0u);
        mask = (uint32_t)(cap - 1);
    }
    void insert(uint64_t hash) {  // (the fill is spread over the pool: racing threads claim a slot by compare-and-swap)
        std::atomic<uint32_t> *at = reinterpret_cast<std::atomic<uint32_t> *>(slots.data());
        const uint32_t tg = tag_of(hash);
        for (uint32_t q = tg & mask;; q = (q + 1) & mask) {
            uint32_t seen = at[q].load(std::memory_order_relaxed);
            if (seen == tg || (seen == 0u && at[q].compare_exchange_strong(seen, tg, std::memory_order_relaxed)) || seen == tg) break;
        }
    }
    bool maybe(uint64_t hash) const {  // false: no allowed object has this name
        const uint32_t tg = tag_of(hash);
        bool hit = false;
        for (uint32_t q = tg & mask; slots[q] != 0u && !hit; q = (q + 1) & mask) hit = slots[q] == tg;
        return hit;
    }
};

// (a user's reach does not change from one list request to the next: a subject last seen with FEW allowed objects is not resolved for while the device
//  walks -- a third of the pass's work, wasted, for the proxy's ordinary user; one never seen, or seen with MANY, is)
// (the hint, one word of acl_engine::keep_seen: 58 bits of the key's hash | 1 + the bit width of the allowed count the last walk returned, 0 = never seen)
struct ReachHint {
    std::atomic<uint64_t> *slot = nullptr;
    uint64_t key = 0;
    bool known = false;
    uint64_t count = 0;  // (a lower bound of what the last walk allowed)
    void look(acl_engine_t *h, int rt, int pm, int st, uint32_t sub) {
        key = (((uint64_t)sub * 0x9E3779B97F4A7C15ull) ^ ((uint64_t)rt << 40) ^ ((uint64_t)pm << 24) ^ ((uint64_t)st << 8)) | 63ull;
        slot = &h->keep_seen[(key >> 20) & 255u];
        const uint64_t was = slot->load(std::memory_order_relaxed);
        known = (was | 63ull) == key && (was & 63ull) != 0;
        count = known ? ((1ull << ((was & 63ull) - 1)) >> 1) : 0;
    }
    void store(uint64_t allowed) {
        const unsigned width = allowed ? 64u - (unsigned)__builtin_clzll(allowed) : 0u;
        slot->store((key & ~63ull) | std::min(62u, 1u + width), std::memory_order_relaxed);
    }
};

// Phase times of the route on stderr (ACL_DEBUG_KEEP): when the walk and the pass were done, what the pool's chunks of the pass and of the test took.
struct KeepTrace {
    using Clock = std::chrono::steady_clock;
    static bool on() {
        static const bool kTrace = getenv("ACL_DEBUG_KEEP") != nullptr;
        return kTrace;
    }
    static double us_since(Clock::time_point t) { return std::chrono::duration<double, std::micro>(Clock::now() - t).count(); }
    static uint64_t ns(Clock::duration d) { return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(d).count(); }
    Clock::time_point t_0{};  // (set when the route has its constants: KeepCall::prepare)
    double us_walk = 0, us_a = 0, us_fill = 0;
    std::atomic<uint64_t> sum{0}, first{~0ull}, last{0}, test{0};  // (pass chunks: ns inside them, when the first began, when the last ended; test chunks: ns inside them)
    struct Chunk {  // one chunk of the pass, or of the test
        KeepTrace *t;
        const bool of_pass;
        const Clock::time_point c0 = Clock::now();
        Chunk(KeepTrace &tr, bool pass) : t(on() ? &tr : nullptr), of_pass(pass) {}
        ~Chunk() {
            if (!t) return;
            const auto now = Clock::now();
            if (!of_pass) {
                t->test.fetch_add(ns(now - c0));
                return;
            }
            t->sum.fetch_add(ns(now - c0));
            const uint64_t st = ns(c0 - t->t_0), en = ns(now - t->t_0);
            for (uint64_t v = t->first.load(); st < v && !t->first.compare_exchange_weak(v, st);) {}
            for (uint64_t v = t->last.load(); en > v && !t->last.compare_exchange_weak(v, en);) {}
        }
    };
    void print(size_t n, uint64_t count) const {
        if (!on()) return;
        std::fprintf(stderr,
                     "keep route: n %zu allowed %llu | walk %.1f us | walk + pass done at %.1f (chunks: %.1f us in all, first began at %.1f, last ended at %.1f) | "
                     "tags at %.1f | end %.1f (test chunks: %.1f us in all)\n",
                     n, (unsigned long long)count, us_walk, us_a, sum.load() / 1e3, first.load() / 1e3, last.load() / 1e3, us_fill, us_since(t_0), test.load() / 1e3);
    }
};

struct PairRanges {  // (no offsets: every pair is an item of its own)
    const uint32_t *off;
    size_t operator[](size_t i) const { return off ? off[i] : i; }
};

// One call of the route: the request, what is learnt about it phase by phase, and the phases in the order keep_by_reverse_walk (below) runs them.
template <class Items>
struct KeepCall {
    static constexpr uint32_t kUnresolved = 0xFFFFFFFEu, kAbsent = 0xFFFFFFFFu;  // idv[]: not looked up (yet); no object of the type has the name
    // the request
    acl_engine_t *const h;
    const Items &its;
    const size_t n;  // pairs
    const PairRanges item_off;
    const size_t k_items;
    uint8_t *const keep_out, *const pair_perm;
    int32_t *const pair_err;
    const bool pair_form;
    const unsigned workers;
    // the call's constants, from item 0 (resolve_constants)
    int rt = -1, pm = -1, st = -1;
    uint32_t sub = 0;
    bool sub_known = false;
    const ObjectTable *tab = nullptr;
    ReachHint hint;
    bool guess_few = false;
    // per pair: the resource name's hash, and its id once resolved (then, in the test, the pair's outcome)
    uint64_t *hv = nullptr;
    uint32_t *idv = nullptr;
    // the walk's answer
    std::vector<uint32_t> row;
    uint64_t count = 0;
    int walk_rc = ACL_OK;
    // (pair form on a snapshot with DEEP objects -- a cycle of groups behind some resources: no_object_is_deep hands over their bitmap; a pair whose bit is missing
    //  answers the depth error when its resource is one of them, so every name goes to the table: never "few")
    std::shared_ptr<const std::vector<uint32_t>> deep;
    const uint32_t *dbits = nullptr;
    size_t dwords = 0;
    std::atomic<bool> walk_done{false}, many_a{false}, resolved_any{false};
    std::atomic<int> outcome{0};  // 0 fine; 1: not a uniform call after all / an item the forward path must judge -> not taken
    bool few = false;             // (after the walk) the test goes through `tags`
    TagSet tags;
    KeepTrace tr;

    KeepCall(acl_engine_t *h_, const Items &its_, size_t n_, const uint32_t *item_off_p, size_t k_items_, uint8_t *keep_out_, uint8_t *pair_perm_, int32_t *pair_err_)
        : h(h_), its(its_), n(n_), item_off{item_off_p}, k_items(k_items_), keep_out(keep_out_), pair_perm(pair_perm_), pair_err(pair_err_), pair_form(keep_out_ == nullptr),
          workers(pool_workers(h_, n_)) {}

    void emit(size_t it, uint8_t all) const {
        if (!pair_form) keep_out[it] = all;
        else {
            pair_perm[it] = all ? ACL_PERM_HAS_PERMISSION : ACL_PERM_NO_PERMISSION;
            pair_err[it] = 0;
        }
    }
    bool is_few(uint64_t allowed) const { return !dbits && allowed != 0 && allowed <= std::max<uint64_t>(kFewFloor, n / kFewShare); }

    // a look at three pairs before any lock is taken or a reverse snapshot asked for: most bulk requests that are not one user's are not at first sight
    bool looks_uniform() const {
        for (size_t i : {(size_t)1, n / 2, n - 1})
            if (!same_constants(its, i)) return false;
        return true;
    }

    // the call's constants, from item 0.  Caller holds names_mu shared.  false: not a call for this route
    bool resolve_constants() {
        if (!h->store.has_schema()) return false;
        NameMemo m;
        int32_t err = 0;
        if (!intern_names(h->store.schema(), its, 0, m, &err) || m.sri != kNoRelation) return false;
        rt = m.rti, pm = m.pmi, st = m.sti;
        const char *u = its.ptr(0, F_SID);
        const std::string_view sid = u ? std::string_view(u, its.len(0, F_SID)) : std::string_view();
        if (sid.empty() || sid == "*" || !valid_object_id(sid)) return false;
        sub_known = h->store.objects(st).find(sid, &sub);
        if (sub_known) h->store.touch(st, sub);  // (the id leaves the names lock: its recycling quarantine starts over, store.hpp)
        tab = &h->store.objects(rt);
        return true;
    }

    // the per-pair arrays, and what the last walk for this subject says about its reach.  false: a short list for a far-reaching subject -- forward
    bool prepare() {
        tr.t_0 = KeepTrace::Clock::now();
        static thread_local std::vector<uint64_t> hv_buf;  // (per calling thread: 512 KB of fresh pages per 65 536-item call cost more than the pass itself)
        if (hv_buf.size() < n) hv_buf.resize(n);
        hv = hv_buf.data();
        static thread_local std::vector<uint32_t> idv_buf;
        if (idv_buf.size() < n) idv_buf.resize(n);
        idv = idv_buf.data();
        if (sub_known) hint.look(h, rt, pm, st, sub);  // (a subject no table knows has no id to remember a reach under: no hint, nothing guessed)
        guess_few = hint.known && (hint.count == 0 || is_few(hint.count));
        // A SHORT list for a subject who reaches thousands of objects: the walk (60-90 us: it marks all of them) costs more than the forward path's pass over
        // the few pairs (1 024 pairs: 0.10 against 0.06 ms).  Not taken then -- except every sixteenth time, so that the hint follows a user whose reach shrinks.
        return !(sub_known && hint.count >= kShortListReach && n < kShortListPairs && (h->keep_route_skips.fetch_add(1, std::memory_order_relaxed) & kShortListRetry) != kShortListRetry);
    }

    // may the row answer this call, and what else it needs: the deep objects' bitmap (pair form), a zeroed row.  false: forward.  c: the evaluation's context
    bool prepare_row(PassCtx *c) {
        const uint32_t target = (uint32_t)h->store.schema().slot(rt, pm);
        // a permission some `&` / `-` can change: forward, whoever asks (a subject no table knows too: what `a - b` gives it is the Check's to say)
        if (h->snap.slot_nonmono.size() > target && h->snap.slot_nonmono[target]) return false;
        // a subject no table knows is answered without a walk -- unless a `st:*` relationship covers it, as it covers every plain subject of the type: forward
        if (!sub_known && store_holds_wildcard_of(st)) return false;
        // (the pair form also for a subject no table knows: a walk through a cycle of groups ends at the depth limit whoever is looked for)
        if (pair_form && (h->snap.slot_deep.size() <= target || (h->snap.slot_deep[target] && !no_object_is_deep(h, c, rt, pm, st, n, &deep)))) return false;
        dbits = deep ? deep->data() : nullptr;
        dwords = deep ? deep->size() : 0;
        if (sub_known) {
            const size_t words = ((size_t)h->store.objects(rt).count() + 31) / 32;
            row.assign(std::max<size_t>(words, 1), 0u);
        }
        return true;
    }

    // "Some relationship of the STORE names `st:*`" (caller holds state_mu shared).  The table's "*" object proves nothing: it is interned with the schema and
    // stays when its last relationship goes.  An expired relationship not collected yet still counts: forward is always right.
    bool store_holds_wildcard_of(int stype) const {
        if (h->store.wildcard_id(stype) == 0xFFFFFFFFu) return false;  // (no relation of the schema allows `stype:*`)
        const Schema &sc = h->store.schema();
        const auto &tables = h->store.tables();
        for (int slot = 0; slot < sc.nslots; slot++) {
            const auto &cls = sc.defs[sc.slot_owner[slot].first].members[sc.slot_owner[slot].second].classes;
            for (size_t k = 0; k < cls.size(); k++)
                if (cls[k].wildcard && cls[k].stype == stype && (!tables[slot][k].keys.empty() || !tables[slot][k].pending.empty())) return true;
        }
        return false;
    }

    // the reverse walk.  None for a subject no table knows: it has no relationships, and without a subject relation it is nobody's member -- so nothing is
    // allowed, PROVIDED no `st:*` relationship covers it: prepare_row has sent such a call forward (the wildcard's row grants whoever is of the type)
    void walk(PassCtx *c) {
        const auto t_w = KeepTrace::Clock::now();
        if (sub_known) walk_rc = lookup_batch(h, c, rt, pm, st, -1, &sub, 1, row.data(), row.size(), &count);
        tr.us_walk = KeepTrace::us_since(t_w);
        many_a.store(dbits || (count != 0 && !is_few(count)), std::memory_order_relaxed);
        walk_done.store(true, std::memory_order_release);
        if (sub_known && !walk_rc) hint.store(count);
    }

    // ... and, while the device still walks (or once it is known that MANY objects are allowed: every name goes to the table then), the pass also RESOLVES the
    // names it has just hashed -- one block of 64 behind the block whose slots it asks for, the names' bytes still in this thread's cache -- so that the test
    // after the walk is a bit test per pair.  A walk that is back with FEW allowed objects stops that: the rest is tested through the tags, no table involved.
    void resolve_block(size_t lo, size_t le) {
        if (le == lo) return;
        const bool back = walk_done.load(std::memory_order_acquire);
        if (back ? many_a.load(std::memory_order_relaxed) : !guess_few) {
            if (!resolved_any.load(std::memory_order_relaxed)) resolved_any.store(true, std::memory_order_relaxed);
            uint32_t rid_loc[kPairBlock];
            for (size_t i = lo; i < le; i++) {
                uint32_t id;
                rid_loc[i - lo] = tab->find_hashed(std::string_view(its.ptr(i, F_RID), its.len(i, F_RID)), hv[i], &id) ? id : kAbsent;
            }
            for (size_t i = lo; i < le; i++) idv[i] = rid_loc[i - lo];
        }
    }

    // The host's pass over the pairs of items [a, b), while the device walks: constants compared with item 0 (by pointer, then by content), the resource name
    // validated and hashed.  The walk is a launch, 30-90 us of kernel and the row's way back; the pass is ~17 ns per pair and thread (30 when it resolves the
    // names too): they overlap, the caller waiting for the device, the pool's workers on the pairs (the caller joins them when the row is back).
    // (both passes go over ITEMS, each worker through its items' pairs [item_off[a], item_off[b]): the keep bytes are then written where they are computed)
    void pass(size_t a, size_t b) {
        KeepTrace::Chunk ct(tr, true);
        // Blocks of 64 items, stage by stage: the offsets; every pair's constant fields and resource id judged; the ids hashed into a LOCAL array; the hashes
        // copied out and their table slots asked for.  (Fused into one loop per pair -- judge, hash, store -- the same work measured 85 cycles per pair
        // instead of 50 on the box's EPYC, 30 of them on the store into the shared array between a pair's loads: rdtsc per stage, round 6.)
        constexpr size_t kBlock = kPairBlock;
        uint64_t loc[kBlock];
        size_t prev_lo = 0, prev_le = 0;  // the block whose slots were asked for last: resolved while the next block's are on their way
        for (size_t g = a; g < b; g += kBlock) {
            if (outcome.load(std::memory_order_relaxed)) return;
            const size_t ge = std::min(b, g + kBlock);
            bool fine = true;
            for (size_t it = g; it < ge; it++) fine &= item_off[it] <= item_off[it + 1] && item_off[it + 1] <= n;  // (else not an ascending offset array: the caller's check says so)
            if (!fine) {
                outcome.store(1, std::memory_order_relaxed);
                return;
            }
            for (size_t lo = item_off[g], hi = item_off[ge]; lo < hi; lo += kBlock) {
                const size_t le = std::min(hi, lo + kBlock);
                for (size_t i = lo; i < le; i++) {
                    const char *r = its.ptr(i, F_RID);
                    const std::string_view rid = r ? std::string_view(r, its.len(i, F_RID)) : std::string_view();
                    fine &= same_constants(its, i) && !rid.empty() && rid != "*" && valid_object_id(rid);  // (else the forward path knows what to do with it: per-item error, whole-call failure, ...)
                }
                if (!fine) {
                    outcome.store(1, std::memory_order_relaxed);
                    return;
                }
                for (size_t i = lo; i < le; i++) loc[i - lo] = ObjectTable::hash_of(std::string_view(its.ptr(i, F_RID), its.len(i, F_RID)));
                for (size_t i = lo; i < le; i++) {
                    hv[i] = loc[i - lo];
                    idv[i] = kUnresolved;
                    tab->prefetch2(loc[i - lo]);
                }
                resolve_block(prev_lo, prev_le);
                prev_lo = lo;
                prev_le = le;
            }
        }
        resolve_block(prev_lo, prev_le);  // (the chunk's last block: one exposed trip per 1 024 pairs)
    }

    // the walk and the pass, side by side from 2 048 items on (from 512 when the pool's workers are still polling after the previous call: intern_items)
    void walk_and_pass(PassCtx *c) {
        InternPool *const P = intern_pool(h, k_items >= kSpreadMin);
        const bool spread = k_items >= kSpreadMin || (k_items >= kSpreadHotMin && P && P->awake());
        if (!spread) {
            walk(c);
            pass(0, k_items);
            return;
        }
        const std::function<void()> walk_fn = [this, c] { walk(c); };
        const std::function<void(size_t, size_t)> pass_fn = [this](size_t a, size_t b) { pass(a, b); };
        P->run(k_items, pool_piece(k_items), workers, pass_fn, &walk_fn);
    }

    // Two ways to test a name against the row.  FEW allowed objects (is_few: at most a thirty-second of the pairs): their names' hash tags make a small set that
    // stays in cache, and only a tag hit goes on to the name table.  MANY: every name goes to the table (one miss, prefetched a group ahead) -- still
    // half of what the forward path's interning pays (it resolves the subject too) and no device pass over K items.
    // false: an allowed object has no name (anonymous ids -- bulk-loaded numeric graphs -- have no names to compare with: forward path)
    bool build_tags() {
        few = is_few(count);
        if (!few) return true;
        tags.reset(count);
        std::atomic<bool> anonymous{false};
        const std::function<void(size_t, size_t)> fill = [&](size_t wa, size_t wb) {
            for (size_t w = wa; w < wb; w++)
                for (uint32_t mbits = row[w]; mbits; mbits &= mbits - 1) {
                    const std::string *nm = tab->name((uint32_t)(w * 32 + (size_t)__builtin_ctz(mbits)));
                    if (!nm) {
                        anonymous.store(true, std::memory_order_relaxed);
                        return;
                    }
                    tags.insert(ObjectTable::hash_of(*nm));
                }
        };
        if (count < kTagFillSpreadMin) fill(0, row.size());
        else intern_pool(h, true)->run(row.size(), std::max<size_t>(256, row.size() / 64), workers, fill);
        return !anonymous.load();
    }

    bool row_bit(uint32_t id) const { return (size_t)(id >> 5) < row.size() && ((row[id >> 5] >> (id & 31u)) & 1u); }

    // (nothing was resolved: tags only, straight into the keep bytes)
    void test_by_tags(size_t a, size_t b) const {
        for (size_t it = a; it < b; it++) {
            uint8_t all = 1;
            for (size_t i = item_off[it]; i < item_off[it + 1]; i++) {
                const uint64_t hh = hv[i];
                uint32_t id;
                all &= (uint8_t)(tags.maybe(hh) && tab->find_hashed(std::string_view(its.ptr(i, F_RID), its.len(i, F_RID)), hh, &id) && row_bit(id));
            }
            emit(it, all);
        }
    }

    // ---- the pairs of items [a, b) against the row; an item is kept when every one of its pairs is (one without pairs too: postfilter.go:145-150).  A pair the pass has
    // resolved is a bit test; one it has not goes through the tags (FEW) and, on a tag hit or with MANY allowed, to the name table -- blocks of 64 pairs, the
    // outcomes into a local array first, then into the ids' place.
    void test(size_t a, size_t b) {
        KeepTrace::Chunk ct(tr, false);
        if (few && !resolved_any.load(std::memory_order_relaxed)) return test_by_tags(a, b);
        constexpr size_t kBlock = kPairBlock;
        const size_t p_lo = item_off[a], p_hi = item_off[b];
        uint8_t ok[kBlock];
        for (size_t lo = p_lo; lo < p_hi; lo += kBlock) {
            const size_t le = std::min(p_hi, lo + kBlock);
            if (!few)
                for (size_t i = lo; i < le; i++)
                    if (idv[i] == kUnresolved) tab->prefetch2(hv[i]);
            for (size_t i = lo; i < le; i++) {
                uint32_t id = idv[i];
                if (id == kUnresolved) {
                    const uint64_t hh = hv[i];
                    // (the name table has the last word: id, then the row's bit)
                    if (!(few ? tags.maybe(hh) : true) || !tab->find_hashed(std::string_view(its.ptr(i, F_RID), its.len(i, F_RID)), hh, &id)) id = kAbsent;
                }
                ok[i - lo] = id != kAbsent && row_bit(id);
                if (dbits && !ok[i - lo] && id != kAbsent && (size_t)(id >> 5) < dwords && ((dbits[id >> 5] >> (id & 31u)) & 1u)) ok[i - lo] = 2;  // (gave up at the depth limit)
            }
            for (size_t i = lo; i < le; i++) idv[i] = ok[i - lo];
        }
        for (size_t it = a; it < b; it++) {
            if (pair_form && idv[it] == 2u) {  // (pair form: item it IS pair it)
                pair_perm[it] = 0;
                pair_err[it] = ACL_ERR_DEPTH;
                continue;
            }
            uint8_t all = 1;
            for (size_t i = item_off[it]; i < item_off[it + 1]; i++) all &= (uint8_t)idv[i];
            emit(it, all);
        }
    }

    void test_all() {
        if (!count && !dbits) {  // (nothing is allowed: only an item without pairs is kept)
            for (size_t it = 0; it < k_items; it++) emit(it, item_off[it] == item_off[it + 1]);
            return;
        }
        InternPool *const P = k_items < kSpreadHotMin ? nullptr : intern_pool(h, k_items >= kSpreadMin);
        if (!P) return test(0, k_items);
        const std::function<void(size_t, size_t)> test_fn = [this](size_t a, size_t b) { test(a, b); };
        P->run(k_items, pool_piece(k_items), workers, test_fn);  // (its workers polled through the walk)
    }
};

}  // namespace

template <class Items>
int keep_by_reverse_walk(acl_engine_t *h, const Items &its, size_t n, const uint32_t *item_off_p, size_t k_items, uint8_t *keep_out, uint8_t *pair_perm, int32_t *pair_err,
                         const CallOpts &opts, Eval *outer) {
    // PAIR form (CheckBulkPermissions itself, keep_out == NULL): every pair is an "item" of its own and is answered HAS_PERMISSION / NO_PERMISSION without an
    // error -- only where no Check of the permission can end in a depth error: whatever the relationships are (Snapshot::slot_deep says so of the schema), or, for a
    // recursive permission, on THIS snapshot (no_object_is_deep) -- because the row's missing bit cannot tell "no" from "gave up at the depth limit", which the
    // forward path reports per pair.
    static const size_t kMin = [] {
        const char *e = getenv("ACL_KEEP_ROUTE_MIN");  // (A/B and test knob; 0 switches the route off)
        return e ? (size_t)std::max(0, atoi(e)) : kRouteMinPairs;
    }();
    if (!kMin || n < kMin || h->store_only || h->shard.world > 1) return kRouteNotTaken;
    KeepCall<Items> k(h, its, n, item_off_p, k_items, keep_out, pair_perm, pair_err);
    if (!k_items || k.item_off[0] != 0 || k.item_off[k_items] != n) return kRouteNotTaken;  // (pairs outside every item: the forward path checks them all the same)
    if (!k.looks_uniform()) return kRouteNotTaken;
    // (state_mu -- the evaluation's -- then names_mu: engine_internal.hpp's order.  The evaluation begins BEFORE the call's constants are resolved: no schema
    //  reload can come between the ids taken here and the walk that uses them.  The names stay locked while the device walks: the pass resolves names then.)
    // (outer: the caller's evaluation -- a K x F call answers its F templates one after the other on ONE snapshot, keep_by_reverse_walks)
    Eval own;
    Eval &ev = outer ? *outer : own;
    if (!outer) {
        int rc = ev.begin(h, true, opts);
        if (rc) return rc;
    }
    std::shared_lock<std::shared_mutex> nlk(h->names_mu);
    if (!k.resolve_constants() || !k.prepare() || !k.prepare_row(ev.c)) return kRouteNotTaken;
    k.walk_and_pass(ev.c);
    if (k.walk_rc) return k.walk_rc;
    if (k.outcome.load()) return kRouteNotTaken;
    k.tr.us_a = KeepTrace::us_since(k.tr.t_0);
    if (!outer) ev.end();
    if (!k.build_tags()) return kRouteNotTaken;
    k.tr.us_fill = KeepTrace::us_since(k.tr.t_0);
    k.test_all();
    if (!outer) h->keep_route_calls.fetch_add(1, std::memory_order_relaxed);  // (a K x F call counts its F walks once all of them have answered)
    k.tr.print(n, k.count);
    return ACL_OK;
}

// K items x F templates (postfilter.go:86-119: every PostFilter of every matching rule, resolved per item -- F = 2 ... 4 here): pair j of every item comes from
// template j, so the pairs at positions j, j + F, j + 2 F, ... are a one-template call of their own.  Each is answered by its reverse walk (EveryNth: a view of
// the call's items) under ONE evaluation -- one snapshot for the whole request, as the forward path has -- and an item is kept when every template keeps it.
// Anything else -- items with different numbers of pairs, a template position whose pairs do not share type / permission / subject, a route that declines --
// returns kRouteNotTaken before keep_out is touched.
template <class Items>
struct EveryNth {
    const Items &base;
    size_t stride, phase;
    static constexpr bool kHasLen = Items::kHasLen;
    const char *ptr(size_t i, int f) const { return base.ptr(i * stride + phase, f); }
    size_t len(size_t i, int f) const { return base.len(i * stride + phase, f); }
};
template <class Items>
static int keep_by_reverse_walks(acl_engine_t *h, const Items &its, size_t n, const uint32_t *item_off, size_t k_items, uint8_t *keep_out) {
    if (!k_items || n % k_items || h->store_only || h->shard.world > 1) return kRouteNotTaken;
    const size_t F = n / k_items;
    if (F < kMultiMinTemplates || F > kMultiMaxTemplates || k_items < kMultiMinItems) return kRouteNotTaken;
    for (size_t i = 0; i <= k_items; i++)
        if (item_off[i] != i * F) return kRouteNotTaken;
    Eval ev;
    int rc = ev.begin(h, true, CallOpts());
    if (rc) return rc;
    {   // F walks must beat ONE forward pass over K F pairs: over a type of a few hundred thousand objects a walk is 20-40 us and they do from a few hundred
        // items on; over C4's 845 000 pods a walk is 30-85 us and two of them (0.21 ms at 16 384 items) beat the forward string path (0.27 ms) from there on
        // (profiles/r06_keep_route.txt) -- such types from 16 384 items on
        std::shared_lock<std::shared_mutex> nlk(h->names_mu);
        if (!h->store.has_schema()) return kRouteNotTaken;
        size_t biggest = 0;
        for (size_t j = 0; j < F; j++) {
            const char *t = its.ptr(j, F_RT);
            const int rt = t ? h->store.schema().type_of(std::string(t, its.len(j, F_RT))) : -1;
            if (rt < 0) return kRouteNotTaken;
            biggest = std::max<size_t>(biggest, h->store.objects(rt).count());
        }
        static const size_t kBigMin = getenv("ACL_KEEP_MULTI_MIN") ? (size_t)std::max(0, atoi(getenv("ACL_KEEP_MULTI_MIN"))) : kMultiBigMinItems;  // (A/B knob)
        if (biggest > kMultiBigType && k_items < kBigMin) return kRouteNotTaken;
    }
    std::vector<uint8_t> kj(F * k_items);
    for (size_t j = 0; j < F; j++) {
        const EveryNth<Items> view{its, F, j};
        rc = keep_by_reverse_walk(h, view, k_items, nullptr, k_items, kj.data() + j * k_items, nullptr, nullptr, CallOpts(), &ev);
        if (rc) return rc;  // (kRouteNotTaken among them)
    }
    ev.end();
    h->keep_route_calls.fetch_add(F, std::memory_order_relaxed);
    for (size_t i = 0; i < k_items; i++) {
        uint8_t all = 1;
        for (size_t j = 0; j < F; j++) all &= kj[j * k_items + i];
        keep_out[i] = all;
    }
    return ACL_OK;
}

template <class Items>
static int check_bulk_keep_strings(acl_engine_t *h, const Items &its, size_t n, const uint32_t *item_off, size_t k_items, uint8_t *keep_out, const char *who) {
    int rc = keep_by_reverse_walk(h, its, n, item_off, k_items, keep_out, nullptr, nullptr, CallOpts());  // (checks the offsets it uses as it goes, in parallel; anything irregular comes back here)
    if (rc == kRouteNotTaken) rc = keep_by_reverse_walks(h, its, n, item_off, k_items, keep_out);  // (K x F: one walk per template)
    if (rc != kRouteNotTaken) return rc;
    for (size_t i = 0; i < k_items; i++)
        if (item_off[i] > item_off[i + 1] || item_off[i + 1] > n) return fail(ACL_ERR_INVALID_ARGUMENT, std::string(who) + ": item_off must ascend and end within n");
    std::vector<uint8_t> perm(std::max<size_t>(n, 1));
    std::vector<int32_t> err(std::max<size_t>(n, 1));
    rc = check_bulk_strings(h, its, n, perm.data(), err.data());
    if (rc) return rc;
    for (size_t i = 0; i < k_items; i++) {
        bool all = true;  // pair error or anything but HAS_PERMISSION drops the item: postfilter.go:162-172
        for (uint32_t j = item_off[i]; j < item_off[i + 1]; j++) all = all && !err[j] && perm[j] == ACL_PERM_HAS_PERMISSION;
        keep_out[i] = all ? 1 : 0;
    }
    return ACL_OK;
}
static int packed_ok(acl_engine_t *h, const acl_packed_request_t *rq, const char *who) {
    if (!rq || (rq->n_items && (!rq->items || !rq->offsets || !rq->bytes))) return fail(ACL_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL buffer");
    const size_t n6 = rq->n_items * 6;
    // (one pass over 24 bytes per item: nothing below reads a string through an index it has not seen; large requests share it out)
    std::atomic<uint32_t> worst_a{0};
    const std::function<void(size_t, size_t)> scan = [&](size_t a, size_t b) {
        uint32_t wv = 0;
        for (size_t k = a; k < b; k++) {
            const uint32_t v = rq->items[k];
            wv = std::max(wv, v == ACL_PACKED_NONE ? 0u : v + 1u);
        }
        uint32_t seen = worst_a.load(std::memory_order_relaxed);
        while (wv > seen && !worst_a.compare_exchange_weak(seen, wv, std::memory_order_relaxed)) {
        }
    };
    if (rq->n_items < 16384) {
        scan(0, n6);
    } else {
        intern_pool(h, true)->run(n6, 6 * 4096, std::min(16u, h->intern_threads) - 1, scan);
    }
    const uint32_t worst = worst_a.load();
    if (worst > rq->n_strings) return fail(ACL_ERR_INVALID_ARGUMENT, std::string(who) + ": a dictionary index lies beyond n_strings");
    return ACL_OK;  // (an absent member -- ACL_PACKED_NONE -- is the pair's own InvalidArgument, as a {NULL, 0} view is)
}
int check_bulk_packed_call(acl_engine_t *h, const acl_packed_request_t *rq, uint8_t *perm_out, int32_t *err_out, const acl_call_opts_t *opts) {
    if (int rc = packed_ok(h, rq, "acl_check_bulk_packed")) return rc;
    if (rq->n_items && (!perm_out || !err_out)) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_check_bulk_packed: NULL buffer");
    return check_bulk_strings(h, PackedItems{rq}, rq->n_items, perm_out, err_out, opts);
}
int check_bulk_keep_packed_call(acl_engine_t *h, const acl_packed_request_t *rq, const uint32_t *item_off, size_t k_items, uint8_t *keep_out) {
    if (int rc = packed_ok(h, rq, "acl_check_bulk_keep_packed")) return rc;
    if (k_items && (!item_off || !keep_out)) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_check_bulk_keep_packed: NULL buffer");
    return check_bulk_keep_strings(h, PackedItems{rq}, rq->n_items, item_off, k_items, keep_out, "acl_check_bulk_keep_packed");
}
int check_bulk_keep_cstr_call(acl_engine_t *h, const acl_check_item_t *items, size_t n, const uint32_t *item_off, size_t k_items, uint8_t *keep_out) {
    if ((n && !items) || (k_items && (!item_off || !keep_out))) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_check_bulk_keep: NULL buffer");
    return check_bulk_keep_strings(h, CStrItems{items}, n, item_off, k_items, keep_out, "acl_check_bulk_keep");
}
int check_bulk_keep_v_call(acl_engine_t *h, const acl_check_item_v_t *items, size_t n, const uint32_t *item_off, size_t k_items, uint8_t *keep_out) {
    if ((n && !items) || (k_items && (!item_off || !keep_out))) return fail(ACL_ERR_INVALID_ARGUMENT, "acl_check_bulk_keep_v: NULL buffer");
    return check_bulk_keep_strings(h, ViewItems{items}, n, item_off, k_items, keep_out, "acl_check_bulk_keep_v");
}


// the item forms check_bulk_strings (engine_intern.cpp) calls the route with
template int keep_by_reverse_walk<CStrItems>(acl_engine_t *, const CStrItems &, size_t, const uint32_t *, size_t, uint8_t *, uint8_t *, int32_t *, const CallOpts &, Eval *);
template int keep_by_reverse_walk<ViewItems>(acl_engine_t *, const ViewItems &, size_t, const uint32_t *, size_t, uint8_t *, uint8_t *, int32_t *, const CallOpts &, Eval *);
template int keep_by_reverse_walk<PackedItems>(acl_engine_t *, const PackedItems &, size_t, const uint32_t *, size_t, uint8_t *, uint8_t *, int32_t *, const CallOpts &, Eval *);

}  // namespace aclint

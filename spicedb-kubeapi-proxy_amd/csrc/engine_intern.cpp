// engine_intern.cpp -- strings -> ids: one item (intern_check_item), bulk requests through the interning pool (intern_items),
// what an invalid item is told, and the string Check entry points' core (check_bulk_strings).
#include "engine_strings.hpp"

namespace aclint {

bool empty(const char *s) { return !s || !*s; }

FilterText to_filter(const acl_filter_t *f) {
    FilterText o;
    o.op = f->op;
    o.rtype = f->resource_type ? f->resource_type : "";
    if (f->resource_id) { o.has_rid = true; o.rid = f->resource_id; }
    if (f->relation) { o.has_rel = true; o.rel = f->relation; }
    if (f->subject_type) { o.has_stype = true; o.stype = f->subject_type; }
    if (f->subject_id) { o.has_sid = true; o.sid = f->subject_id; }
    if (f->subject_relation) { o.has_srel = true; o.srel = f->subject_relation; }
    return o;
}

int32_t intern_check_item(acl_engine_t *h, const acl_check_item_t &it, acl_item_t *out) {
    const Schema &sc = h->store.schema();
    if (empty(it.resource_type) || empty(it.resource_id) || empty(it.permission) || empty(it.subject_type) || empty(it.subject_id))
        return ACL_ERR_INVALID_ARGUMENT;  // empty request: pkg/proxy/options_test.go:101-102
    int rt = sc.type_of(it.resource_type), st = sc.type_of(it.subject_type);
    int pm = rt < 0 ? -1 : sc.defs[rt].find(it.permission);
    int sr = kNoRelation;
    bool bad = rt < 0 || st < 0 || pm < 0;
    const bool srel_given = !empty(it.subject_relation) && std::strcmp(it.subject_relation, "...") != 0;
    if (srel_given) {
        sr = st < 0 ? -1 : sc.defs[st].find(it.subject_relation);
        bad = bad || sr < 0;
    }
    // API validation beats "not found" (validate.hpp): ill-formed names and ids, and `*` anywhere in a Check
    if ((rt < 0 && !valid_type_name(it.resource_type)) || (st < 0 && !valid_type_name(it.subject_type)) || (pm < 0 && !valid_relation_name(it.permission)) ||
        (srel_given && sr < 0 && !valid_relation_name(it.subject_relation)))
        return ACL_ERR_INVALID_ARGUMENT;
    if (bad) {
        if (!valid_object_id(it.resource_id) || !valid_object_id(it.subject_id)) return ACL_ERR_INVALID_ARGUMENT;
        return ACL_ERR_FAILED_PRECONDITION;
    }
    // unknown object ids have no relationships: sentinels above every dense id, equal only when
    // resource and subject are the same (unknown) object
    uint32_t res, sub;
    bool kr = h->store.objects(rt).find(it.resource_id, &res), ks = h->store.objects(st).find(it.subject_id, &sub);
    // (these ids leave the names lock in the caller's hands -- a single Check queued in the batcher: their recycling quarantine starts over, store.hpp touch)
    if (kr) h->store.touch(rt, res);
    if (ks) h->store.touch(st, sub);
    // (every name IN a table passed the id pattern when it was interned -- except "*", the wildcard subject's name: only unknown ids are spelled out)
    if ((!kr && !valid_object_id(it.resource_id)) || (!ks && !valid_object_id(it.subject_id)) || std::strcmp(it.resource_id, "*") == 0 || std::strcmp(it.subject_id, "*") == 0)
        return ACL_ERR_INVALID_ARGUMENT;
    if (!kr && !ks && rt == st && std::strcmp(it.resource_id, it.subject_id) == 0) res = sub = 0xFFFFFFFEu;
    else {
        if (!kr) res = 0xFFFFFFFDu;
        if (!ks) sub = 0xFFFFFFFCu;
    }
    *out = acl_item_t{(uint16_t)rt, (uint16_t)pm, res, (uint16_t)st, (uint16_t)(sr == kNoRelation ? ACL_NO_RELATION : sr), sub};
    return 0;
}

// Which field of item i fails the API's validation, and why -- for acl_last_error() ("check failed" told an operator nothing; the
// reference denies everything a failed CheckBulkPermissions asked, pkg/authz/check.go:48-52, so the message is all there is to diagnose a blanket denial).
template <class Items>
static std::string describe_invalid(const Schema &sc, const Items &its, size_t i) {
    static const char *const kField[6] = {"resource type", "resource id", "permission", "subject type", "subject id", "subject relation"};
    auto view = [&](int f) {
        const char *q = its.ptr(i, f);
        return q ? std::string_view(q, its.len(i, f)) : std::string_view();
    };
    auto shown = [](std::string_view v) {
        std::string o(v.substr(0, 48));
        for (char &ch : o)
            if ((unsigned char)ch < 0x20 || (unsigned char)ch > 0x7E) ch = '?';
        return "`" + o + (v.size() > 48 ? "...` (" + std::to_string(v.size()) + " bytes)" : "`");
    };
    const std::string_view rt = view(F_RT), rid = view(F_RID), pm = view(F_PM), st = view(F_ST), sid = view(F_SID);
    std::string_view sr = view(F_SR);
    if (sr == "...") sr = std::string_view();
    const int rti = sc.type_of(std::string(rt)), sti = sc.type_of(std::string(st));
    auto bad_id = [&](int f, std::string_view v) -> std::string {
        if (v.empty()) return std::string(kField[f]) + " is empty";
        if (v == "*") return std::string(kField[f]) + " `*`: a wildcard is not an object of a Check";
        if (v.size() > 1024) return std::string(kField[f]) + " " + shown(v) + " is longer than 1024 bytes";
        size_t at = 0;
        while (at < v.size() && valid_object_id(v.substr(at, 1))) at++;
        if (at < v.size()) return std::string(kField[f]) + " " + shown(v) + " does not match ^[a-zA-Z0-9/_|\\-=+]{1,1024}$ (byte " + std::to_string(at) + " `" +
                                  ((unsigned char)v[at] >= 0x20 && (unsigned char)v[at] <= 0x7E ? std::string(1, v[at]) : std::string("?")) + "`)";
        return std::string();
    };
    if (rt.empty()) return "resource type is empty";
    if (rti < 0 && !valid_type_name(rt)) return "resource type " + shown(rt) + " does not match ^([a-z][a-z0-9_]{1,61}[a-z0-9]/)*[a-z][a-z0-9_]{1,62}[a-z0-9]$";
    if (std::string e = bad_id(F_RID, rid); !e.empty()) return e;
    if (pm.empty()) return "permission is empty";
    if ((rti < 0 || sc.defs[rti].find(std::string(pm)) < 0) && !valid_relation_name(pm)) return "permission " + shown(pm) + " does not match ^[a-z][a-z0-9_]{1,62}[a-z0-9]$";
    if (st.empty()) return "subject type is empty";
    if (sti < 0 && !valid_type_name(st)) return "subject type " + shown(st) + " does not match ^([a-z][a-z0-9_]{1,61}[a-z0-9]/)*[a-z][a-z0-9_]{1,62}[a-z0-9]$";
    if (std::string e = bad_id(F_SID, sid); !e.empty()) return e;
    if (!sr.empty() && (sti < 0 || sc.defs[sti].find(std::string(sr)) < 0) && !valid_relation_name(sr))
        return "subject relation " + shown(sr) + " does not match ^[a-z][a-z0-9_]{1,62}[a-z0-9]$ (or empty, or `...`)";
    return "a field is empty or ill-formed";
}
template <class Items>
static int fail_invalid_item(acl_engine_t *h, const Items &its, size_t i) {
    std::shared_lock<std::shared_mutex> nlk(h->names_mu);
    return fail(ACL_ERR_INVALID_ARGUMENT, "invalid CheckBulkPermissionsRequest: item " + std::to_string(i) + ": " + describe_invalid(h->store.schema(), its, i));
}

void intern_pool_destroy(acl_engine_t *h) {
    delete h->intern_pool;
    h->intern_pool = nullptr;
}

// (the one place that clamps hardware_concurrency(); intern_threads is at least 2)
unsigned host_threads(acl_engine_t *h) { return std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), h->intern_threads); }

InternPool *intern_pool(acl_engine_t *h, bool create) {
    std::lock_guard<std::mutex> lk(h->intern_pool_mu);
    if (!h->intern_pool && create) h->intern_pool = new InternPool(std::max(2u, host_threads(h)) - 1);
    return h->intern_pool;
}
size_t pool_piece(size_t n) { return n >= 32768 ? 1024 : n >= 8192 ? 512 : n >= 2048 ? 128 : 64; }
// threads per batch: 16 up to 32 767 items, 32 beyond (same-box A/B on a 256-thread host, profiles/r03_string_path_ab.txt: 65 536 named
// items 135 -> 170 M decisions/s with 32; 16 384 items the same with either, 48 threads slower at both sizes)
unsigned pool_workers(acl_engine_t *h, size_t n) { return (n >= 32768 ? h->intern_threads : std::min(16u, h->intern_threads)) - 1; }

// fn over [0, total) in pieces, on the interning pool's threads and the caller (engine_list.cpp: a list response's bytes).  Lock order as for the interning
// callers: names_mu (shared) may be held, state_mu must not be waited for inside fn.
void host_parallel(acl_engine_t *h, size_t total, size_t piece, const std::function<void(size_t, size_t)> &fn) {
    piece = std::max<size_t>(piece, 1);
    if (host_threads(h) <= 1 || total <= piece) {
        if (total) fn(0, total);
        return;
    }
    intern_pool(h, true)->run(total, piece, h->intern_threads - 1, fn);
}
// Interns n items into `out` (the evaluation context's pinned staging: what the H2D copy reads).  An item that cannot be checked -- empty
// field, unknown type / permission / relation: the pair carries an error, check.go:55 -- becomes a DEAD item (the kernel answers it
// "invalid" without touching the graph) and is listed in *bad with its error; the batch is never compacted or copied again.
template <class Items>
void intern_items(acl_engine_t *h, const Items &its, size_t n, acl_item_t *out, std::vector<std::pair<uint32_t, int32_t>> *bad, bool ids_leave_the_call) {
    const Schema &sc = h->store.schema();
    std::mutex bad_mu;
    // Packed requests: a name that many items of the call carry -- the namespace of every pod of a list, the user of every pair -- is looked up ONCE: entry d of
    // this table remembers what dictionary string d resolved to as an object of one type ((type + 1) << 33 | known << 32 | id; 0 = not yet; racing threads store the
    // same value).  Items that name an object for the first time pay the table's DRAM miss as before.
    constexpr bool kPacked = std::is_same_v<Items, PackedItems>;
    std::unique_ptr<std::atomic<uint64_t>[]> dict_cache;
    if constexpr (kPacked) {
        // (only where the dictionary says names REPEAT: a call of K distinct resources and one user has about one string per item, and a table that is
        //  zeroed, filled and never hit cost the 65 536-item call 60 us)
        if (n >= 64 && (size_t)its.rq->n_strings * 2 <= n) {
            dict_cache.reset(new std::atomic<uint64_t>[its.rq->n_strings]);
            for (uint32_t d = 0; d < its.rq->n_strings; d++) dict_cache[d].store(0, std::memory_order_relaxed);
        }
    }
    auto cached = [&](size_t i, int f, int type, bool *known, uint32_t *id) -> bool {
        if constexpr (kPacked) {
            if (!dict_cache) return false;
            const uint64_t v = dict_cache[its.idx(i, f)].load(std::memory_order_relaxed);
            if ((v >> 33) != (uint64_t)type + 1u) return false;
            *known = (v >> 32) & 1u;
            *id = (uint32_t)v;
            return true;
        } else {
            (void)i, (void)f, (void)type, (void)known, (void)id;
            return false;
        }
    };
    auto remember = [&](size_t i, int f, int type, bool known, uint32_t id) {
        if constexpr (kPacked) {
            if (dict_cache) dict_cache[its.idx(i, f)].store(((uint64_t)type + 1u) << 33 | (uint64_t)known << 32 | id, std::memory_order_relaxed);
        } else {
            (void)i, (void)f, (void)type, (void)known, (void)id;
        }
    };
    // Object ids: two lookups per item in tables of up to millions of names -- two dependent DRAM misses each (slot, then the name's
    // bytes).  Items go in groups of kGroup through three stages: hash + prefetch the slots; walk to the tag match + prefetch the names;
    // compare.  The misses of a group are in flight together.
    constexpr size_t kGroup = 16;  // (32: no better on the GPU box's host; prefetching the NEXT group's id bytes ahead of their hashing: 0.33 against 0.32 ms per 65 536 items, not kept -- tools/intern_bench.py)
    static const bool kPieces = getenv("ACL_DEBUG_INTERN_PIECES") != nullptr;
    const int64_t tp0 = kPieces ? mono_ns() : 0;
    std::atomic<int64_t> p_sum{0}, p_first{INT64_MAX}, p_last{0}, p_max{0};
    std::atomic<int> p_threads{0};
    const std::function<void(size_t, size_t)> run = [&](size_t a, size_t b) {
        struct PieceTrace {
            int64_t t0, c0;
            std::atomic<int64_t> *sum, *first, *last, *mx;
            ~PieceTrace() {
                if (!sum) return;
                const int64_t now = mono_ns();
                sum->fetch_add(now - c0);
                for (int64_t v = first->load(); c0 - t0 < v && !first->compare_exchange_weak(v, c0 - t0);) {}
                for (int64_t v = last->load(); now - t0 > v && !last->compare_exchange_weak(v, now - t0);) {}
                for (int64_t v = mx->load(); now - c0 > v && !mx->compare_exchange_weak(v, now - c0);) {}
            }
        } pt{tp0, kPieces ? mono_ns() : 0, kPieces ? &p_sum : nullptr, &p_first, &p_last, &p_max};
        static thread_local int64_t seen_call = 0;
        if (kPieces && seen_call != tp0) { seen_call = tp0; p_threads.fetch_add(1); }
        NameMemo m;
        std::vector<std::pair<uint32_t, int32_t>> mybad;
        const int64_t touch_ms = ids_leave_the_call ? Store::steady_now_ms() : 0;  // (one clock read per chunk, not per id)
        struct Pending {
            uint64_t hr, hs;
            std::string_view rid, sid;
            int rt, st, pm, sr;
            bool ok;
            bool same_res, same_sub;  // the same object as the item before it: its id is taken over, not looked up again
            bool hit_res, hit_sub;    // packed requests: the dictionary entry was resolved earlier in this call (kr / res, ks / sub already hold the answer)
            bool kr, ks;              // (third stage) the table knows the name
            uint32_t res, sub;
        } pend[kGroup];
        // The proxy's batches repeat themselves: every pair of a PostFilter call names the requesting user (postfilter.go:88-119), the F templates
        // of a list item name the same object one after the other, check.go:17-72 builds all of a request's pairs for one user.  A name equal
        // to the previous item's (same type; pointer + length, or content) costs no hash, no prefetch and no probe.
        Pending last{};  // the last item of the previous group that resolved
        bool have_last = false;
        auto same_name = [](std::string_view x, std::string_view y) { return x.size() == y.size() && (x.data() == y.data() || std::memcmp(x.data(), y.data(), x.size()) == 0); };
        for (size_t g0 = a; g0 < b; g0 += kGroup) {
            const size_t g1 = std::min(b, g0 + kGroup);
            for (size_t i = g0; i < g1; i++) {
                Pending &p = pend[i - g0];
                int32_t err = 0;
                const char *r = its.ptr(i, F_RID), *u = its.ptr(i, F_SID);
                p.rid = r ? std::string_view(r, its.len(i, F_RID)) : std::string_view();
                p.sid = u ? std::string_view(u, its.len(i, F_SID)) : std::string_view();
                p.ok = intern_names(sc, its, i, m, &err);
                // an empty or ill-formed id beats an unknown name (API validation comes first); ids of items that resolve are spelled out
                // only where the table does not know them (third stage below: every name IN a table passed the pattern when it was interned)
                if (err != ACL_ERR_INVALID_ARGUMENT && (p.rid.empty() || p.sid.empty() || (!p.ok && (!valid_object_id(p.rid) || !valid_object_id(p.sid))))) {
                    p.ok = false;
                    err = ACL_ERR_INVALID_ARGUMENT;
                }
                if (!p.ok) {
                    out[i] = acl_item_t{kDeadType, 0, 0, kDeadType, 0, 0};
                    mybad.emplace_back((uint32_t)i, err);
                    continue;
                }
                p.rt = m.rti; p.st = m.sti; p.pm = m.pmi; p.sr = m.sri;
                const Pending *prev = i > g0 && pend[i - g0 - 1].ok ? &pend[i - g0 - 1] : (i == g0 && have_last ? &last : nullptr);
                p.same_res = prev && prev->rt == p.rt && same_name(prev->rid, p.rid);
                p.same_sub = prev && prev->st == p.st && same_name(prev->sid, p.sid);
                p.hit_res = !p.same_res && cached(i, F_RID, p.rt, &p.kr, &p.res);  // (packed requests: this dictionary entry was resolved earlier in the call)
                p.hit_sub = !p.same_sub && cached(i, F_SID, p.st, &p.ks, &p.sub);
                if (p.hit_res) p.same_res = false;
                if (p.hit_sub) p.same_sub = false;
                if (p.hit_res && p.hit_sub) continue;
                if (!p.same_res && !p.hit_res) {
                    p.hr = ObjectTable::hash_of(p.rid);
                    h->store.objects(p.rt).prefetch(p.hr);
                }
                if (!p.same_sub && !p.hit_sub) {
                    p.hs = ObjectTable::hash_of(p.sid);
                    h->store.objects(p.st).prefetch(p.hs);
                }
            }
            for (size_t i = g0; i < g1; i++) {
                const Pending &p = pend[i - g0];
                if (!p.ok) continue;
                if (!p.same_res && !p.hit_res) h->store.objects(p.rt).prefetch_name(p.hr);
                if (!p.same_sub && !p.hit_sub) h->store.objects(p.st).prefetch_name(p.hs);
            }
            for (size_t i = g0; i < g1; i++) {
                Pending &p = pend[i - g0];
                if (!p.ok) continue;
                // unknown object ids have no relationships: sentinels above every dense id, equal only when
                // resource and subject are the same (unknown) object
                const Pending *prev = i > g0 ? &pend[i - g0 - 1] : &last;  // (same_res / same_sub were only set against an item that resolved)
                if (p.same_res) p.kr = prev->kr, p.res = prev->res;
                else if (!p.hit_res) {
                    p.kr = h->store.objects(p.rt).find_hashed(p.rid, p.hr, &p.res);
                    remember(i, F_RID, p.rt, p.kr, p.res);
                }
                if (p.same_sub) p.ks = prev->ks, p.sub = prev->sub;
                else if (!p.hit_sub) {
                    p.ks = h->store.objects(p.st).find_hashed(p.sid, p.hs, &p.sub);
                    remember(i, F_SID, p.st, p.ks, p.sub);
                }
                const bool kr = p.kr, ks = p.ks;
                uint32_t res = p.res, sub = p.sub;
                if (ids_leave_the_call) {  // (acl_resolve_bulk_v: the recycling quarantine of an unreferenced object starts over, store.hpp touch)
                    if (kr && !p.same_res) h->store.touch(p.rt, res, touch_ms);
                    if (ks && !p.same_sub) h->store.touch(p.st, sub, touch_ms);
                }
                if ((!kr && !valid_object_id(p.rid)) || (!ks && !valid_object_id(p.sid)) || p.rid == "*" || p.sid == "*") {  // (`*` never in a Check)
                    out[i] = acl_item_t{kDeadType, 0, 0, kDeadType, 0, 0};
                    mybad.emplace_back((uint32_t)i, (int32_t)ACL_ERR_INVALID_ARGUMENT);
                    continue;
                }
                if (!kr && !ks && p.rt == p.st && p.rid == p.sid) res = sub = 0xFFFFFFFEu;
                else {
                    if (!kr) res = 0xFFFFFFFDu;
                    if (!ks) sub = 0xFFFFFFFCu;
                }
                out[i] = acl_item_t{(uint16_t)p.rt, (uint16_t)p.pm, res, (uint16_t)p.st, (uint16_t)(p.sr == kNoRelation ? ACL_NO_RELATION : p.sr), sub};
            }
            have_last = pend[g1 - g0 - 1].ok;  // (the next group's first item is compared with this group's last one)
            if (have_last) last = pend[g1 - g0 - 1];
        }
        if (!mybad.empty()) {
            std::lock_guard<std::mutex> lk(bad_mu);
            bad->insert(bad->end(), mybad.begin(), mybad.end());
        }
    };
    // tens of nanoseconds per item on one thread: below 4 096 items waking the pool up (20-100 us per sleeping thread) costs more than it saves -- unless its
    // workers are still polling after the previous batch (a busy proxy's calls follow each other within that window): then from 512 items on
    bool hot = false;
    if (n >= 512 && n < 4096) {
        const InternPool *P = intern_pool(h, false);
        hot = P && P->awake();
    }
    if (n < 4096 && !hot) {
        run(0, n);
        return;
    }
    intern_pool(h, true)->run(n, pool_piece(n), pool_workers(h, n), run);
    if (kPieces) std::fprintf(stderr, "intern pieces of %zu items: %d threads, %.1f us inside pieces in all (longest %.1f), first began at %.1f, last ended at %.1f, back at %.1f\n", n, p_threads.load(), p_sum.load() / 1e3, p_max.load() / 1e3, p_first.load() / 1e3, p_last.load() / 1e3, (mono_ns() - tp0) / 1e3);
}

// acl_check_bulk / acl_check_bulk_v: strings -> ids straight into the context's pinned staging, one device pass, per-item errors patched in
template <class Items>
int check_bulk_strings(acl_engine_t *h, const Items &its, size_t n, uint8_t *perm_out, int32_t *err_out, const acl_call_opts_t *o) {
    if (!n) return h->store_only ? fail(ACL_ERR_UNAVAILABLE, "engine was opened store-only (no GPU): Check / LookupResources are unavailable") : ACL_OK;
    const CallOpts opts = call_opts(o);  // (cancellation / deadline: honoured while the call waits for an evaluation context, as in acl_check_bulk_ids_opts)
    // A request whose pairs all name ONE plain subject, one type and one permission -- what filterItemsWithBulkPermissions sends for a list
    // (postfilter.go:67-134) -- is answered by one reverse walk + bit tests when the permission allows it (keep_by_reverse_walk, pair form); anything else
    // comes back here before a byte was written.
    {
        const int rrc = keep_by_reverse_walk(h, its, n, nullptr, n, nullptr, perm_out, err_out, opts);
        if (rrc != kRouteNotTaken) return rrc;
    }
    Eval ev;
    int rc = ev.begin(h, false, opts);
    if (rc) return rc;
    PassCtx *c = ev.c;
    std::vector<std::pair<uint32_t, int32_t>> bad;
    HIP_TRY(c->h_in.ensure(n * sizeof(acl_item_t)));
    acl_item_t *staged = (acl_item_t *)c->h_in.p;
    static const bool kTimeIt = getenv("ACL_DEBUG_STRING_TIMING") != nullptr;  // (stderr: where a string call's time goes -- tools/string_path.py)
    const int64_t t_a = kTimeIt ? mono_ns() : 0;
    {
        std::shared_lock<std::shared_mutex> nlk(h->names_mu);  // string -> id only reads the tables: concurrent callers intern in parallel
        if (!h->store.has_schema()) return fail(ACL_ERR_FAILED_PRECONDITION, "no schema loaded");
        intern_items(h, its, n, staged, &bad);
    }
    const int64_t t_b = kTimeIt ? mono_ns() : 0;
    // A request that fails the API's validation fails AS A WHOLE with InvalidArgument -- no pairs at all (validate.hpp; the reference denies
    // everything it asked on any error of the call, check.go:48-52, and fails the list response, postfilter.go:134-137).  Unknown types /
    // permissions stay per-item errors (check.go:55-60).
    for (const auto &be : bad)
        if (be.second == ACL_ERR_INVALID_ARGUMENT && !h->per_item_validation) return fail_invalid_item(h, its, be.first);
    if (bad.size() == n) {  // nothing to ask the device
        std::memset(perm_out, ACL_PERM_UNSPECIFIED, n);
    } else {
        rc = check_ids_host(h, c, staged, n, perm_out, err_out);
        if (rc) return rc;
    }
    if (kTimeIt && n >= 1024) fprintf(stderr, "[aclgpu] string call of %zu items: begin %.1f us, interning %.1f us, device pass %.1f us\n", n, 0.0, (t_b - t_a) / 1e3, (mono_ns() - t_b) / 1e3);
    for (const auto &be : bad) {
        perm_out[be.first] = ACL_PERM_UNSPECIFIED;
        err_out[be.first] = be.second;
    }
    return ACL_OK;
}

// the item forms the other translation units call these with
template void intern_items<ViewItems>(acl_engine_t *, const ViewItems &, size_t, acl_item_t *, std::vector<std::pair<uint32_t, int32_t>> *, bool);
template int check_bulk_strings<CStrItems>(acl_engine_t *, const CStrItems &, size_t, uint8_t *, int32_t *, const acl_call_opts_t *);
template int check_bulk_strings<ViewItems>(acl_engine_t *, const ViewItems &, size_t, uint8_t *, int32_t *, const acl_call_opts_t *);
template int check_bulk_strings<PackedItems>(acl_engine_t *, const PackedItems &, size_t, uint8_t *, int32_t *, const acl_call_opts_t *);

}  // namespace aclint

